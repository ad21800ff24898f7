"""ctypes binding of libradarays_mi355.so (include/radarays_mi355.h).

This is the ONLY compute path of the package: if the library is missing or no
HIP device is usable, everything here raises -- there is no CPU fallback.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RADARAYS_MI355_LIB") or os.path.join(_HERE, "libradarays_mi355.so")
_LIB = None

class RRMaterial(C.Structure):
    _fields_ = [("velocity", C.c_float), ("ambient", C.c_float),
                ("diffuse", C.c_float), ("specular", C.c_float)]


class RRConfig(C.Structure):
    _fields_ = [
        ("n_cells", C.c_int32), ("n_angles", C.c_int32), ("n_reflections", C.c_int32),
        ("signal_denoising", C.c_int32),
        ("signal_denoising_triangular_width", C.c_int32),
        ("signal_denoising_gaussian_width", C.c_int32),
        ("signal_denoising_mb_width", C.c_int32),
        ("ambient_noise", C.c_int32), ("scroll_image", C.c_int32),
        ("record_multi_reflection", C.c_int32), ("record_multi_path", C.c_int32),
        ("max_waves_per_azimuth", C.c_int32), ("brdf_model", C.c_int32), ("reserved_", C.c_int32),
        ("resolution", C.c_double), ("energy_max", C.c_double), ("signal_max", C.c_double),
        ("signal_denoising_triangular_mode", C.c_double),
        ("signal_denoising_gaussian_mode", C.c_double),
        ("signal_denoising_mb_mode", C.c_double),
        ("ambient_noise_at_signal_0", C.c_double), ("ambient_noise_at_signal_1", C.c_double),
        ("ambient_noise_energy_max", C.c_double), ("ambient_noise_energy_min", C.c_double),
        ("ambient_noise_energy_loss", C.c_double), ("multipath_threshold", C.c_double),
        ("wave_energy_threshold", C.c_float), ("theta_min", C.c_float),
        ("theta_inc", C.c_float), ("range_max", C.c_float),
    ]


class RRParamSet(C.Structure):
    _fields_ = [("materials", C.c_void_p), ("beam_dirs", C.c_void_p), ("n_reflections", C.c_int32), ("reserved_", C.c_int32)]


class RRMesh(C.Structure):
    _fields_ = [("verts", C.POINTER(C.c_float)), ("n_verts", C.c_size_t), ("faces", C.POINTER(C.c_uint32)), ("n_faces", C.c_size_t),
                ("face_object_id", C.POINTER(C.c_uint32)), ("n_objects", C.c_size_t), ("object_names", C.POINTER(C.c_char_p))]


class RRDetectConfig(C.Structure):
    _fields_ = [("method", C.c_int32), ("guard_cells", C.c_int32), ("train_cells", C.c_int32), ("k", C.c_int32),
                ("min_intensity", C.c_int32), ("min_bin", C.c_int32), ("cfar_scale", C.c_float), ("reserved_", C.c_int32)]


class RRWindowDetectConfig(C.Structure):
    _fields_ = [("method", C.c_int32), ("guard_range", C.c_int32), ("train_range", C.c_int32), ("guard_azimuth", C.c_int32),
                ("train_azimuth", C.c_int32), ("rank_permille", C.c_int32), ("min_intensity", C.c_int32), ("min_bin", C.c_int32),
                ("scale", C.c_float), ("reserved_", C.c_int32 * 3)]


class RRCartesianConfig(C.Structure):
    _fields_ = [("width", C.c_int32), ("interpolation", C.c_int32), ("pixel_size", C.c_float), ("reserved_", C.c_int32)]


# ---- records: the numpy dtype is the one statement of each; its ctypes Structure (RR*) is derived from it.
# rr_echo as numpy sees it (8 B): one record of an echo stream of rr_debug_column
ECHO_DTYPE = np.dtype([("cell", "<i4"), ("strength", "<f4")])

# rr_echo_src as numpy sees it (16 B): an echo and where it came from (rr_simulate_provenance); LABEL_NONE = RR_LABEL_NONE
ECHO_SRC_DTYPE = np.dtype([("cell", "<i4"), ("strength", "<f4"), ("face", "<u4"), ("info", "<u4")])
LABEL_NONE = 0xFFFFFFFF
LABEL_MAX_CELLS = 8192


def unpack_info(info):
    """the info word of an echo or a label pixel -> (object id, pass, kind); kind 0: path echo, 1: multipath echo.  Arrays or scalars;
    RR_LABEL_NONE unpacks to (0xFFFFFF, 15, 1) with the unused top bits set: mask such pixels with `info != LABEL_NONE` first."""
    i = np.asarray(info, np.uint32)
    return i & np.uint32(0xFFFFFF), (i >> np.uint32(24)) & np.uint32(15), (i >> np.uint32(28)) & np.uint32(1)


# rr_object_note as numpy sees it (80 B): one record per (frame, object) of rr_annotate_labels; the classes of a labelled pixel
NOTE_DTYPE = np.dtype([("n_direct", "<u4"), ("n_ghost", "<u4"), ("n_multipath", "<u4"), ("n_extent", "<u4"), ("bin_min", "<u4"), ("bin_max", "<u4"),
                       ("az_begin", "<u4"), ("az_count", "<u4"), ("peak", "<u4"), ("peak_bin", "<u4"), ("peak_az", "<u4"), ("reserved0_", "<u4"),
                       ("sum_intensity", "<u8"), ("x_min", "<f4"), ("x_max", "<f4"), ("y_min", "<f4"), ("y_max", "<f4"), ("reserved1_", "<u4", (2,))])
NOTE_DIRECT, NOTE_GHOST, NOTE_MULTIPATH = 1, 2, 4
NOTE_ALL = NOTE_DIRECT | NOTE_GHOST | NOTE_MULTIPATH
NOTE_NAMES = {"direct": NOTE_DIRECT, "ghost": NOTE_GHOST, "multipath": NOTE_MULTIPATH}


RRObjectNote = np.ctypeslib.as_ctypes_type(NOTE_DTYPE)


def note_mask(extent):
    """an extent mask -> its bits: an int 0..7, a class name ("direct", "ghost", "multipath") or a list of names; ValueError otherwise"""
    if isinstance(extent, str):
        extent = [extent]
    if isinstance(extent, (list, tuple, set, frozenset)):
        m = 0
        for name in extent:
            if not isinstance(name, str) or name not in NOTE_NAMES:
                raise ValueError("unknown pixel class %r (direct, ghost, multipath)" % (name,))
            m |= NOTE_NAMES[name]
        return m
    return _int_in(extent, 0, NOTE_ALL, "extent_mask")


# rr_wave_rec as numpy sees it (64 B): one ray-cast wave of an azimuth's wave list (rr_simulate_paths); WavRec is the same record for ctypes
WAVE_DTYPE = np.dtype([("o", "<f4", (3,)), ("range", "<f4"), ("d", "<f4", (3,)), ("face", "<u4"), ("energy", "<f8"), ("time", "<f8"),
                       ("info", "<u4"), ("parent", "<i4"), ("material", "<u4"), ("echo", "<i4")])
WAVES_MAP_FRAME = 1
WAVES_MAX_PASSES = 16
RRWaveRec = np.ctypeslib.as_ctypes_type(WAVE_DTYPE)

# rr_radar_point as numpy sees it (24 B: a PointCloud's point + its intensity channel, and where it came from)
POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4"), ("column", "<u4"), ("bin", "<u4")])
RRRadarPoint = np.ctypeslib.as_ctypes_type(POINT_DTYPE)

# rr_sweep_rec as numpy sees it (32 B): one azimuth's transform into the reference frame and its Doppler range shift
SWEEP_DTYPE = np.dtype([("q", "<f4", (4,)), ("t", "<f4", (3,)), ("dr", "<f4")])
RRSweepRec = np.ctypeslib.as_ctypes_type(SWEEP_DTYPE)


def identity_sweep_table(n_frames, n_angles):
    """SWEEP_DTYPE [n_frames][n_angles] that compensates nothing: q = (0, 0, 0, 1), t = 0, dr = 0"""
    t = np.zeros((int(n_frames), int(n_angles)), SWEEP_DTYPE)
    t["q"][..., 3] = 1.0
    return t


# rr_icp_rec as numpy sees it (48 B): the state (c, s, tx, ty) that maps a source point into the target's frame, and the last pass's score
ICP_DTYPE = np.dtype([("c", "<f8"), ("s", "<f8"), ("tx", "<f8"), ("ty", "<f8"), ("sse", "<i8"), ("n_matched", "<u4"), ("flags", "<u4")])
ICP_DEGENERATE, ICP_TRUNCATED = 1, 2
ICP_NONE = 0xFFFFFFFF              # an unmatched point in the correspondences
ICP_MAX_POINTS = 65536
RRIcpRec = np.ctypeslib.as_ctypes_type(ICP_DTYPE)


def se2_states(yaw, tx=0.0, ty=0.0):
    """planar transforms as rr_register_points takes them: float64 [n][4] = (cos yaw, sin yaw, tx, ty); scalars or arrays that broadcast"""
    yaw, tx, ty = np.broadcast_arrays(np.atleast_1d(np.asarray(yaw, np.float64)), np.asarray(tx, np.float64), np.asarray(ty, np.float64))
    return np.ascontiguousarray(np.stack([np.cos(yaw), np.sin(yaw), tx, ty], axis=1))


def icp_tile_sizes():
    """(source points per workgroup, target points per LDS tile) of k_icp_pass"""
    a, b = C.c_int(0), C.c_int(0)
    lib().rr_icp_tile_sizes(C.byref(a), C.byref(b))
    return a.value, b.value


def _icp_gate(gate):
    """the gate as the library takes it (f32): finite and positive, also after rounding"""
    try:
        g = float(gate)
    except (TypeError, ValueError):
        raise ValueError("gate must be a number, got %r" % (gate,))
    with np.errstate(over="ignore"):
        g32 = np.float32(g)
    if isinstance(gate, bool) or not (np.isfinite(g32) and g32 > 0):
        raise ValueError("gate must be finite and > 0 as a float32, got %r" % (gate,))
    return float(g32)


def _icp_init(init, n):
    """None or float64 [n][4] with a finite non-zero (c, s) in every row"""
    if init is None:
        return None
    x = _states(init, np.float64, "init", n=n)
    h = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1])
    if not np.all(np.isfinite(h) & (h > 0)):
        raise ValueError("every initial state needs a finite, non-zero (c, s)")
    return x


# ---- likelihood field (rr_field.hip).  rr_field_rec as numpy sees it (16 B): the score of one pose hypothesis
FIELD_DTYPE = np.dtype([("sum_d2", "<u8"), ("n_in", "<u4"), ("n_hit", "<u4")])
FIELD_MAX_SIDE, FIELD_MAX_DIST, FIELD_MAX_HYP = 4096, 255, 1 << 22
RRFieldRec = np.ctypeslib.as_ctypes_type(FIELD_DTYPE)


class RRFieldConfig(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("cell", C.c_float), ("x0", C.c_float), ("y0", C.c_float),
                ("max_dist", C.c_int32), ("gate", C.c_int32), ("reserved_", C.c_int32)]


def _f32_finite(v, what, positive=False):
    """a number that is finite (and > 0) as a float32 -> that float32 as a Python float"""
    try:
        with np.errstate(over="ignore"):
            g = np.float32(float(v))
    except (TypeError, ValueError):
        raise ValueError("%s must be a number, got %r" % (what, v))
    if isinstance(v, bool) or not np.isfinite(g) or (positive and not g > 0):
        raise ValueError("%s must be finite%s as a float32, got %r" % (what, " and > 0" if positive else "", v))
    return float(g)


def field_config(width, height, cell, x0, y0, max_dist=FIELD_MAX_DIST, gate=0):
    """rr_field_config, range-checked before any call into the library: width x height cells of `cell` metres, the low corner of cell
    (0, 0) at (x0, y0) in the map frame, distances saturated at max_dist cells, a point a HIT within gate cells.  An RRFieldConfig passes
    through the same checks."""
    w, h = _int_in(width, 1, FIELD_MAX_SIDE, "width"), _int_in(height, 1, FIELD_MAX_SIDE, "height")
    md = _int_in(max_dist, 1, FIELD_MAX_DIST, "max_dist")
    return RRFieldConfig(w, h, _f32_finite(cell, "cell", True), _f32_finite(x0, "x0"), _f32_finite(y0, "y0"), md, _int_in(gate, 0, md, "gate"), 0)


def _field_cfg(cfg):
    if isinstance(cfg, RRFieldConfig):
        return field_config(cfg.width, cfg.height, cfg.cell, cfg.x0, cfg.y0, cfg.max_dist, cfg.gate)
    if isinstance(cfg, dict):
        return field_config(**cfg)
    raise ValueError("a field config must be an RRFieldConfig (native.field_config makes one) or a dict of its arguments, got %r" % (cfg,))


def field_tile_sizes():
    """(points a wave of k_field_score takes per step, hypotheses per workgroup of it, cells of a row per sweep of the transform's row pass)"""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    lib().rr_field_tile_sizes(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


# ---- occupancy mapping (rr_occupancy.hip).  rr_occupancy_config (32 B): the inverse sensor model of one update
OCC_MAX_EVIDENCE = 127


class RROccupancyConfig(C.Structure):
    _fields_ = [("l_hit", C.c_int32), ("l_free", C.c_int32), ("margin_bins", C.c_int32), ("max_free_bin", C.c_int32), ("reserved_", C.c_int32 * 4)]


def occupancy_config(l_hit, l_free, margin_bins, max_free_bin, n_cells):
    """rr_occupancy_config, range-checked before any call into the library: l_hit (1..127) is added to a cell per detection, l_free (0..127)
    subtracted per scan that saw it empty; margin_bins (0..n_cells) bins in front of an azimuth's first detection stay unknown; free space
    is asserted below max_free_bin (0..n_cells) only, and an azimuth with no detection is free up to it"""
    n = _int_in(n_cells, 1, 1 << 30, "n_cells")
    return RROccupancyConfig(_int_in(l_hit, 1, OCC_MAX_EVIDENCE, "l_hit"), _int_in(l_free, 0, OCC_MAX_EVIDENCE, "l_free"),
                             _int_in(margin_bins, 0, n, "margin_bins"), _int_in(max_free_bin, 0, n, "max_free_bin"), (C.c_int32 * 4)())


def _grid_cfg(cfg):
    """the grid of an occupancy call: an RRFieldConfig or a dict of field_config's arguments whose shape and place are range-checked;
    max_dist and gate are ignored there and pass as they are"""
    if isinstance(cfg, RRFieldConfig):
        g = field_config(cfg.width, cfg.height, cfg.cell, cfg.x0, cfg.y0, 1, 0)
        g.max_dist, g.gate = cfg.max_dist, cfg.gate
        return g
    return _field_cfg(cfg)


def occupancy_tile_sizes():
    """(cells per workgroup of k_occ_free, consecutive cells per thread of it, scans per staged profile chunk -- 0: not chunked)"""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    lib().rr_occupancy_tile_sizes(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


# ---- particle filter step (rr_filter.hip).  rr_filter_config (32 B) and rr_filter_summary (32 B) as numpy sees them
FILTER_CONFIG_DTYPE = np.dtype([("quantum", "<u4"), ("n_table", "<u4"), ("phase", "<u4"), ("seed", "<u4"), ("step", "<u4"), ("sigma_xy", "<f4"),
                                ("sigma_t", "<f4"), ("reserved", "<u4")])
FILTER_SUMMARY_DTYPE = np.dtype([("min_sum_d2", "<u8"), ("total_weight", "<u8"), ("sum_w2", "<u8"), ("best", "<u4"), ("n_unique", "<u4")])
FILTER_MAX_QUANTUM, FILTER_MAX_TABLE, FILTER_MAX_PHASE, FILTER_MAX_N = 1 << 31, 4096, (1 << 24) - 1, 1 << 22
FILTER_VARIATE_STD = float(np.sqrt((65536.0 ** 2 - 1.0) / 3.0))    # of the integer variate: a centred sum of four 16-bit uniforms
RRFilterConfig = np.ctypeslib.as_ctypes_type(FILTER_CONFIG_DTYPE)
RRFilterSummary = np.ctypeslib.as_ctypes_type(FILTER_SUMMARY_DTYPE)


def _f32_scale(v, what):
    g = _f32_finite(v, what)
    if g < 0:
        raise ValueError("%s must be >= 0, got %r" % (what, v))
    return g


def filter_config(sigma_xy_m=0.0, sigma_yaw_rad=0.0, quantum=1, n_table=1, phase=0, seed=0, step=0):
    """rr_filter_config, range-checked before any call into the library.  sigma_xy_m (metres) and sigma_yaw_rad (radians, below pi) are the
    standard deviations of the diffusion; they become per-unit scales of the integer variate here, on the host: divided by
    sqrt((65536^2 - 1) / 3), the angle as tan(yaw / 2).  quantum (1..2^31) sum_d2 units per step of the weight table of n_table
    (1..4096) entries; phase (0..2^24 - 1) where the comb of draws starts; seed and step enter the hash.  An RRFilterConfig is re-checked
    with _filter_cfg."""
    sx, sy = _f32_scale(sigma_xy_m, "sigma_xy_m"), _f32_scale(sigma_yaw_rad, "sigma_yaw_rad")
    if not sy < np.pi:
        raise ValueError("sigma_yaw_rad must be below pi, got %r" % (sigma_yaw_rad,))
    return RRFilterConfig(_int_in(quantum, 1, FILTER_MAX_QUANTUM, "quantum"), _int_in(n_table, 1, FILTER_MAX_TABLE, "n_table"),
                          _int_in(phase, 0, FILTER_MAX_PHASE, "phase"), _int_in(seed, 0, 0xFFFFFFFF, "seed"), _int_in(step, 0, 0xFFFFFFFF, "step"),
                          _f32_scale(sx / FILTER_VARIATE_STD, "sigma_xy"), _f32_scale(np.tan(0.5 * sy) / FILTER_VARIATE_STD, "sigma_t"), 0)


def _filter_cfg(cfg):
    """an RRFilterConfig (filter_config makes one; its fields are held to their ranges again) or a dict of filter_config's arguments"""
    if isinstance(cfg, RRFilterConfig):
        if cfg.reserved != 0:
            raise ValueError("reserved must be 0, got %r" % (cfg.reserved,))
        return RRFilterConfig(_int_in(cfg.quantum, 1, FILTER_MAX_QUANTUM, "quantum"), _int_in(cfg.n_table, 1, FILTER_MAX_TABLE, "n_table"),
                              _int_in(cfg.phase, 0, FILTER_MAX_PHASE, "phase"), cfg.seed, cfg.step, _f32_scale(cfg.sigma_xy, "sigma_xy"),
                              _f32_scale(cfg.sigma_t, "sigma_t"), 0)
    if isinstance(cfg, dict):
        return filter_config(**cfg)
    raise ValueError("a filter config must be an RRFilterConfig (native.filter_config makes one) or a dict of its arguments, got %r" % (cfg,))


def filter_weight_table(sigma_cells, quantum, n_table):
    """the uint16 weight table of rr_filter_resample: table[k] = round(65535 * exp(-k * quantum / (2 sigma^2))) with sigma in cells (sum_d2
    is in squared cells), table[0] at least 1 -- the likelihood of a particle k quanta worse than the best"""
    sg = _f32_finite(sigma_cells, "sigma_cells", True)
    q, nt = _int_in(quantum, 1, FILTER_MAX_QUANTUM, "quantum"), _int_in(n_table, 1, FILTER_MAX_TABLE, "n_table")
    t = np.rint(65535.0 * np.exp(-np.arange(nt, dtype=np.float64) * q / (2.0 * sg * sg))).astype(np.uint16)
    t[0] = max(int(t[0]), 1)
    return t


def filter_tile_sizes():
    """(records per scan tile, draws per workgroup of the draw kernel, entries of cum staged per workgroup -- 0: searched in global memory)"""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    lib().rr_filter_tile_sizes(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def _increment(increment):
    """the odometry increment (Dc, Ds, dx, dy) of rr_filter_move -> four finite float32 values as Python floats; None: the identity"""
    if increment is None:
        return 1.0, 0.0, 0.0, 0.0
    v = np.asarray(increment)
    if v.dtype.kind not in "fiu" or v.shape != (4,):
        raise ValueError("the increment must be four real numbers (Dc, Ds, dx, dy), got %r" % (increment,))
    return tuple(_f32_finite(x, "the increment") for x in v.tolist())


# ---- map refinement (rr_refine.hip): the nearest-cell table of a grid map (uint32 [height][width], NEAREST_NONE where no occupied cell lies
# within max_dist) and scan-to-map ICP from many starting states; the records are ICP_DTYPE
NEAREST_NONE = 0xFFFFFFFF
REFINE_RANGE = 8192.0             # every extent of a refinement's grid must lie within +-REFINE_RANGE metres


def refine_tile_sizes():
    """(points a wave of k_refine takes per step, hypotheses per workgroup of it, cells of a row per sweep of the transform's row pass)"""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    lib().rr_refine_tile_sizes(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def _refine_cfg(cfg):
    """a field config whose four extents, taken in f64 from its f32 fields, lie within +-REFINE_RANGE"""
    g = _field_cfg(cfg)
    for e in (g.x0, g.y0, g.x0 + g.width * float(g.cell), g.y0 + g.height * float(g.cell)):
        if not abs(e) < REFINE_RANGE:
            raise ValueError("the grid of a refinement must lie within +-%g m, an extent is at %r" % (REFINE_RANGE, e))
    return g


def _lattice_axis(half, step, what):
    half, step = float(half), float(step)
    if not (np.isfinite(half) and half >= 0 and np.isfinite(step) and step > 0):
        raise ValueError("%s needs a finite half extent >= 0 and a finite step > 0" % what)
    k = int(np.floor(half / step + 1e-9))
    return np.arange(-k, k + 1, dtype=np.float64) * step


def pose_lattice(center_xy_yaw, half_extent_xy, step_xy, half_yaw, step_yaw):
    """the hypotheses of a dense search around (x, y, yaw): every node of the lattice centre + (i * step_xy, j * step_xy, k * step_yaw) with
    |i * step_xy| <= half_extent_xy and |k * step_yaw| <= half_yaw (radians), x slowest, yaw fastest, so the centre is the middle node.
    Returns (states float32 [n][4] = (cos yaw, sin yaw, x, y) as rr_score_poses takes them: the scan's sensor frame into the map frame,
    xyz float64 [n][3] = the nodes).  cos and sin are numpy's in float64, rounded once to float32: the states are inputs of the scoring,
    so this does not touch its bit-exactness."""
    c = np.asarray(center_xy_yaw, np.float64).reshape(-1)
    if c.shape != (3,) or not np.all(np.isfinite(c)):
        raise ValueError("the centre must be three finite numbers (x, y, yaw), got %r" % (center_xy_yaw,))
    dxy, dyaw = _lattice_axis(half_extent_xy, step_xy, "the xy lattice"), _lattice_axis(half_yaw, step_yaw, "the yaw lattice")
    n = len(dxy) * len(dxy) * len(dyaw)
    if n > FIELD_MAX_HYP:
        raise ValueError("a lattice of %d nodes: at most %d hypotheses per call" % (n, FIELD_MAX_HYP))
    gx, gy, gyaw = np.meshgrid(c[0] + dxy, c[1] + dxy, c[2] + dyaw, indexing="ij")
    xyz = np.stack([gx.ravel(), gy.ravel(), gyaw.ravel()], axis=1)
    states = np.stack([np.cos(xyz[:, 2]), np.sin(xyz[:, 2]), xyz[:, 0], xyz[:, 1]], axis=1).astype(np.float32)
    return np.ascontiguousarray(states), xyz


# ---- beam model (rr_cast.hip): rr_beam_config (32 B), and rr_beam_rec as numpy sees it (32 B): one hypothesis' rays against one scan
BEAM_DTYPE = np.dtype([("n_agree", "<u4"), ("n_short", "<u4"), ("n_through", "<u4"), ("n_open", "<u4"), ("n_none", "<u4"), ("n_cast", "<u4"),
                       ("sum_abs", "<u8")])
BEAM_MAX_STEP, BEAM_MAX_CELLS, CAST_MAX_HYP = 64, 65535, 65535
RRBeamRec = np.ctypeslib.as_ctypes_type(BEAM_DTYPE)


class RRBeamConfig(C.Structure):
    _fields_ = [("bin_begin", C.c_int32), ("bin_end", C.c_int32), ("bin_step", C.c_int32), ("tol_bins", C.c_int32), ("clip_bins", C.c_int32),
                ("reserved_", C.c_int32 * 3)]


def beam_config(bin_begin, bin_end, n_cells, bin_step=1, tol_bins=0, clip_bins=0):
    """rr_beam_config, range-checked before any call into the library: a ray samples the bins bin_begin + k * bin_step below bin_end
    (0 <= bin_begin <= bin_end <= n_cells, bin_step 1..64); a measured bin within tol_bins (0..n_cells) of the expected one agrees; one
    azimuth adds at most clip_bins (0..n_cells) to sum_abs"""
    n = _int_in(n_cells, 1, BEAM_MAX_CELLS, "n_cells")
    end = _int_in(bin_end, 0, n, "bin_end")
    return RRBeamConfig(_int_in(bin_begin, 0, end, "bin_begin"), end, _int_in(bin_step, 1, BEAM_MAX_STEP, "bin_step"),
                        _int_in(tol_bins, 0, n, "tol_bins"), _int_in(clip_bins, 0, n, "clip_bins"), (C.c_int32 * 3)())


def beam_directions(cfg):
    """the direction table of the ray calls for an rr_config (make_config returns one, Context._rrcfg holds it): float32 [n_angles][2] =
    (cos, sin) of theta_min + a * theta_inc per azimuth INDEX a, numpy's in float64, rounded once to float32.  Like pose_lattice's states
    the table is an input of the cast, so this does not touch its bit-exactness."""
    theta = float(cfg.theta_min) + np.arange(int(cfg.n_angles), dtype=np.float64) * float(cfg.theta_inc)
    return np.ascontiguousarray(np.stack([np.cos(theta), np.sin(theta)], axis=1).astype(np.float32))


def _cast_cfg(cfg):
    """the grid of a ray call: an RRFieldConfig or a dict of field_config's arguments whose shape, place and max_dist are range-checked;
    gate is ignored there and passes as it is"""
    if isinstance(cfg, RRFieldConfig):
        g = field_config(cfg.width, cfg.height, cfg.cell, cfg.x0, cfg.y0, cfg.max_dist, 0)
        g.gate = cfg.gate
        return g
    return _field_cfg(cfg)


def cast_tile_sizes():
    """(azimuths a wave of k_cast takes per step, hypotheses a wave takes in turn, hypotheses per workgroup)"""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    lib().rr_cast_tile_sizes(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


# ---- mesh maps (rr_slice.hip): rr_slice_config (16 B), the height band of a slice of the scene's triangles into the grid map
OBJECT_NONE = 0xFFFFFFFF          # what an object plane holds where no triangle marks the cell


class RRSliceConfig(C.Structure):
    _fields_ = [("z_lo", C.c_float), ("z_hi", C.c_float), ("flags", C.c_uint32), ("reserved_", C.c_int32)]


def slice_config(z_lo, z_hi):
    """rr_slice_config, range-checked before any call into the library: the band [z_lo, z_hi] in metres of the map frame, both finite as
    float32 and z_lo <= z_hi (equal: a plane)"""
    lo, hi = _f32_finite(z_lo, "z_lo"), _f32_finite(z_hi, "z_hi")
    if lo > hi:
        raise ValueError("z_lo must not exceed z_hi, got %r > %r" % (z_lo, z_hi))
    return RRSliceConfig(lo, hi, 0, 0)


def _slice_cfg(cfg):
    """an RRSliceConfig (slice_config makes one; held to its ranges again) or a (z_lo, z_hi) pair"""
    if isinstance(cfg, RRSliceConfig):
        if cfg.flags != 0:
            raise ValueError("flags must be 0, got %r" % (cfg.flags,))
        return slice_config(cfg.z_lo, cfg.z_hi)
    if isinstance(cfg, (tuple, list)) and len(cfg) == 2:
        return slice_config(*cfg)
    raise ValueError("a slice config must be an RRSliceConfig (native.slice_config makes one) or a (z_lo, z_hi) pair, got %r" % (cfg,))


def slice_tile_sizes():
    """(the largest candidate box, in cells, that a record's own thread tests; the side of a tile of k_slice_large; threads per workgroup)"""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    lib().rr_slice_tile_sizes(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


# ---- connected components (rr_components.hip): rr_components_config (32 B) and rr_component (80 B), one record per kept component
COMPONENT_DTYPE = np.dtype([("root", "<u4"), ("n_pixels", "<u4"), ("row_min", "<u4"), ("row_max", "<u4"), ("col_min", "<u4"), ("col_max", "<u4"),
                            ("col_lo_max", "<u4"), ("col_hi_min", "<u4"), ("peak", "<u4"), ("peak_row", "<u4"), ("peak_col", "<u4"), ("flags", "<u4"),
                            ("sum_intensity", "<u8"), ("sum_row", "<u8"), ("sum_col", "<u8"), ("reserved_", "<u8")])
COMP_SEAM, COMP_BORDER = 1, 2
COMPONENTS_MAX_SIDE, COMPONENTS_MAX_PLANES = 8192, 65535
RRComponent = np.ctypeslib.as_ctypes_type(COMPONENT_DTYPE)


class RRComponentsConfig(C.Structure):
    _fields_ = [("height", C.c_int32), ("width", C.c_int32), ("threshold", C.c_int32), ("connectivity", C.c_int32), ("wrap_x", C.c_int32),
                ("min_pixels", C.c_int32), ("max_components", C.c_int32), ("reserved_", C.c_int32)]


def components_config(height, width, threshold, connectivity=8, wrap_x=False, min_pixels=1, max_components=4096):
    """rr_components_config, range-checked before any call into the library: planes of height x width pixels (1..8192 each), foreground
    iff value >= threshold (1..255), neighbours by connectivity 4 or 8, column width-1 the left neighbour of column 0 with wrap_x (which
    needs width >= 3), components below min_pixels dropped, at most max_components records written per plane (0: counts only)"""
    h, w = _int_in(height, 1, COMPONENTS_MAX_SIDE, "height"), _int_in(width, 1, COMPONENTS_MAX_SIDE, "width")
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError("connectivity must be 4 or 8, got %r" % (connectivity,))
    if not isinstance(wrap_x, (bool, np.bool_)) and wrap_x not in (0, 1):
        raise ValueError("wrap_x must be a bool, got %r" % (wrap_x,))
    if wrap_x and w < 3:
        raise ValueError("wrap_x needs width >= 3, got %d" % w)
    return RRComponentsConfig(h, w, _int_in(threshold, 1, 255, "threshold"), int(connectivity), int(bool(wrap_x)),
                              _int_in(min_pixels, 1, 0x7FFFFFFF, "min_pixels"), _int_in(max_components, 0, 0x7FFFFFFF, "max_components"), 0)


def _components_cfg(cfg):
    """an RRComponentsConfig (components_config makes one; held to its ranges again) or a dict of components_config's arguments"""
    if isinstance(cfg, RRComponentsConfig):
        if cfg.reserved_ != 0:
            raise ValueError("reserved_ must be 0, got %r" % (cfg.reserved_,))
        return components_config(cfg.height, cfg.width, cfg.threshold, cfg.connectivity, cfg.wrap_x, cfg.min_pixels, cfg.max_components)
    if isinstance(cfg, dict):
        return components_config(**cfg)
    raise ValueError("a components config must be an RRComponentsConfig (native.components_config makes one) or a dict of its arguments, got %r" % (cfg,))


def components_tile_sizes():
    """(width, height) in pixels of the tile a workgroup of k_cc_tile labels in LDS"""
    a, b = C.c_int(0), C.c_int(0)
    lib().rr_components_tile_sizes(C.byref(a), C.byref(b))
    return a.value, b.value


# ---- correlative scan matching (rr_correlate.hip): rr_corr_config (32 B) and rr_corr_rec (112 B), the one record of a search
CORR_DTYPE = np.dtype([("rot", "<i4"), ("dx", "<i4"), ("dy", "<i4"), ("flags", "<u4"), ("sum_d2", "<u8"), ("n_in", "<u4"), ("n_hit", "<u4"),
                       ("upper", "<u8"), ("evaluated", "<u4", (9,)), ("kept", "<u4", (9,))])
CORR_OVERFLOW = 1
CORR_MAX_HALF, CORR_MAX_LEVELS, CORR_MAX_ROT, CORR_MAX_CAPACITY, CORR_MAX_NODES = 2047, 8, 4096, 1 << 24, 1 << 31
RRCorrRec = np.ctypeslib.as_ctypes_type(CORR_DTYPE)


class RRCorrConfig(C.Structure):
    _fields_ = [("half_x", C.c_int32), ("half_y", C.c_int32), ("levels", C.c_int32), ("capacity", C.c_int32), ("reserved_", C.c_int32 * 4)]


def corr_config(half_x, half_y, levels=4, capacity=1 << 16):
    """rr_corr_config, range-checked before any call into the library: the window |dx| <= half_x, |dy| <= half_y in cells (0..2047 each),
    top-level candidates 2^levels cells wide (levels 0..8; 0 is the exhaustive search), at most `capacity` candidates per list (1..2^24)"""
    return RRCorrConfig(_int_in(half_x, 0, CORR_MAX_HALF, "half_x"), _int_in(half_y, 0, CORR_MAX_HALF, "half_y"),
                        _int_in(levels, 0, CORR_MAX_LEVELS, "levels"), _int_in(capacity, 1, CORR_MAX_CAPACITY, "capacity"), (C.c_int32 * 4)(0, 0, 0, 0))


def _corr_cfg(cfg, n_rot=None):
    """an RRCorrConfig (corr_config makes one; held to its ranges again) or a dict of corr_config's arguments; with n_rot, the node count too"""
    if isinstance(cfg, RRCorrConfig):
        if any(cfg.reserved_):
            raise ValueError("reserved_ must be 0")
        k = corr_config(cfg.half_x, cfg.half_y, cfg.levels, cfg.capacity)
    elif isinstance(cfg, dict):
        k = corr_config(**cfg)
    else:
        raise ValueError("a search config must be an RRCorrConfig (native.corr_config makes one) or a dict of its arguments, got %r" % (cfg,))
    if n_rot is not None and n_rot * (2 * k.half_x + 1) * (2 * k.half_y + 1) >= CORR_MAX_NODES:
        raise ValueError("%d rotations of a %d x %d window are 2^31 nodes or more" % (n_rot, 2 * k.half_x + 1, 2 * k.half_y + 1))
    return k


def correlate_tile_sizes():
    """(points a wave takes per step, top-level candidates of one row per wave of k_corr_top, parents per wave of k_corr_expand)"""
    a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
    lib().rr_correlate_tile_sizes(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def corr_node(rec, half_x, half_y):
    """the node index of a record's winner: (rot * (2*half_y+1) + dy + half_y) * (2*half_x+1) + dx + half_x"""
    return (int(rec["rot"]) * (2 * half_y + 1) + int(rec["dy"]) + half_y) * (2 * half_x + 1) + int(rec["dx"]) + half_x


# ---- oriented surface points and point-to-line scan matching (rr_surfels.hip): rr_surfel_config (32 B) and rr_surfel (32 B)
SURFEL_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("var_n", "<f4"), ("var_t", "<f4"), ("count", "<u4"), ("cell", "<u4")])
SURFELS_TRUNCATED, SURFELS_CAPPED = 1, 2
SURFELS_MAX_WIDTH, SURFELS_MAX_CELL_Q, SURFELS_MAX_RECORDS = 1024, 4096, 1 << 20
RRSurfel = np.ctypeslib.as_ctypes_type(SURFEL_DTYPE)


class RRSurfelConfig(C.Structure):
    _fields_ = [("cell", C.c_float), ("width", C.c_int32), ("min_points", C.c_int32), ("max_ratio", C.c_float), ("reserved_", C.c_int32 * 4)]


def surfel_cell_q(cell):
    """cell_q = rintf(cell * 256) of a cell size in metres, as the library takes it (f32)"""
    try:
        with np.errstate(over="ignore", invalid="ignore"):
            q = np.rint(np.float32(cell) * np.float32(256.0))
    except (TypeError, ValueError):
        raise ValueError("cell must be a number, got %r" % (cell,))
    if isinstance(cell, bool) or not (np.isfinite(q) and 1 <= q <= SURFELS_MAX_CELL_Q):
        raise ValueError("cell must give rintf(cell * 256) in 1..%d, got %r" % (SURFELS_MAX_CELL_Q, cell))
    return int(q)


def surfel_config(cell, width, min_points=3, max_ratio=0.1):
    """rr_surfel_config, range-checked before any call into the library: square cells of `cell` metres (rintf(cell * 256) in 1..4096),
    `width` cells per side (1..1024) centred on the sensor, a surface point needs min_points (2..65536) points in its 3 x 3 block and
    lambda_min <= max_ratio * lambda_max (max_ratio in 0..1)"""
    surfel_cell_q(cell)
    if isinstance(max_ratio, bool) or not isinstance(max_ratio, (int, float, np.integer, np.floating)) or not 0.0 <= float(np.float32(max_ratio)) <= 1.0:
        raise ValueError("max_ratio must be a number in [0, 1], got %r" % (max_ratio,))
    return RRSurfelConfig(float(np.float32(cell)), _int_in(width, 1, SURFELS_MAX_WIDTH, "width"), _int_in(min_points, 2, 65536, "min_points"),
                          float(np.float32(max_ratio)), (C.c_int32 * 4)(0, 0, 0, 0))


def _surfel_cfg(cfg):
    """an RRSurfelConfig (surfel_config makes one; held to its ranges again) or a dict of surfel_config's arguments"""
    if isinstance(cfg, RRSurfelConfig):
        if any(cfg.reserved_):
            raise ValueError("reserved_ must be 0")
        return surfel_config(cfg.cell, cfg.width, cfg.min_points, cfg.max_ratio)
    if isinstance(cfg, dict):
        return surfel_config(**cfg)
    raise ValueError("a surfel config must be an RRSurfelConfig (native.surfel_config makes one) or a dict of its arguments, got %r" % (cfg,))


def surfels_tile_sizes():
    """(points per workgroup of the binning launch, cells per chunk of the scan) of rr_surfels.hip"""
    a, b = C.c_int(0), C.c_int(0)
    lib().rr_surfels_tile_sizes(C.byref(a), C.byref(b))
    return a.value, b.value


# ---- pose-graph optimisation (rr_graph.hip): rr_graph_edge (48 B), rr_graph_config (32 B) and rr_graph_rec (32 B)
GRAPH_EDGE_DTYPE = np.dtype([("i", "<u4"), ("j", "<u4"), ("c", "<f8"), ("s", "<f8"), ("tx", "<f8"), ("ty", "<f8"), ("w_t", "<f4"), ("w_r", "<f4")])
GRAPH_REC_DTYPE = np.dtype([("chi2", "<f8"), ("n_used", "<u4"), ("n_flipped", "<u4"), ("n_bad", "<u4"), ("n_dead", "<u4"), ("cg_stop", "<i4"),
                            ("reserved_", "<u4")])
GRAPH_EDGE_FLIPPED, GRAPH_EDGE_BAD = 1, 2
GRAPH_MAX_NODES, GRAPH_MAX_EDGES, GRAPH_MAX_ITERATIONS, GRAPH_MAX_CG_ITERATIONS = 1 << 20, 1 << 22, 256, 1024
RRGraphEdge = np.ctypeslib.as_ctypes_type(GRAPH_EDGE_DTYPE)
RRGraphRec = np.ctypeslib.as_ctypes_type(GRAPH_REC_DTYPE)


class RRGraphConfig(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("cg_iterations", C.c_int32), ("lambda", C.c_double), ("robust_k", C.c_double), ("reserved_", C.c_int32 * 2)]


def _graph_real(v, what):
    """a finite real >= 0 as the library takes it (f64)"""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not (np.isfinite(v) and v >= 0):
        raise ValueError("%s must be finite and >= 0, got %r" % (what, v))
    return float(v)


def graph_config(iterations=10, cg_iterations=50, lam=0.0, robust_k=0.0):
    """rr_graph_config, range-checked before any call into the library: `iterations` outer Gauss-Newton iterations (0..256) of
    `cg_iterations` CG steps each (0..1024), `lam` added to the diagonal of H (>= 0; a graph without a fixed node needs > 0),
    robust_k the Cauchy kernel's scale (0: plain least squares)"""
    g = RRGraphConfig(_int_in(iterations, 0, GRAPH_MAX_ITERATIONS, "iterations"), _int_in(cg_iterations, 0, GRAPH_MAX_CG_ITERATIONS, "cg_iterations"),
                      0.0, _graph_real(robust_k, "robust_k"), (C.c_int32 * 2)(0, 0))
    setattr(g, "lambda", _graph_real(lam, "lambda"))
    return g


def _graph_cfg(cfg):
    """an RRGraphConfig (graph_config makes one; held to its ranges again) or a dict of graph_config's arguments"""
    if isinstance(cfg, RRGraphConfig):
        if any(cfg.reserved_):
            raise ValueError("reserved_ must be 0")
        return graph_config(cfg.iterations, cfg.cg_iterations, getattr(cfg, "lambda"), cfg.robust_k)
    if isinstance(cfg, dict):
        return graph_config(**cfg)
    raise ValueError("a graph config must be an RRGraphConfig (native.graph_config makes one) or a dict of its arguments, got %r" % (cfg,))


def graph_edges(i, j, states, w_t=1.0, w_r=1.0):
    """matcher records packed into GRAPH_EDGE_DTYPE [E]: edge k says that node j[k] sits at states[k] in node i[k]'s frame.  states: ICP_DTYPE
    records (rr_register_points, rr_register_surfels or rr_refine_poses with target scan i and source scan j, as they come) or float64
    [E][4] = (c, s, tx, ty); w_t (1/m^2) and w_r: scalars or arrays that broadcast"""
    i, j = np.atleast_1d(np.asarray(i)), np.atleast_1d(np.asarray(j))
    if i.ndim != 1 or i.shape != j.shape or i.dtype.kind not in "iu" or j.dtype.kind not in "iu":
        raise ValueError("i and j must be integer arrays of one length")
    if len(i) and (min(i.min(), j.min()) < 0 or max(i.max(), j.max()) > 0xFFFFFFFF):
        raise ValueError("a node index must fit 32 bits")
    st = np.asarray(states)
    if st.dtype == ICP_DTYPE:
        st = np.stack([st[k] for k in ("c", "s", "tx", "ty")], axis=-1)
    st = np.asarray(st, np.float64).reshape(-1, 4)
    if len(st) != len(i):
        raise ValueError("one state per edge: %d states for %d edges" % (len(st), len(i)))
    e = np.zeros(len(i), GRAPH_EDGE_DTYPE)
    e["i"], e["j"] = i, j
    e["c"], e["s"], e["tx"], e["ty"] = st[:, 0], st[:, 1], st[:, 2], st[:, 3]
    e["w_t"], e["w_r"] = np.broadcast_to(np.asarray(w_t, np.float32), e.shape), np.broadcast_to(np.asarray(w_r, np.float32), e.shape)
    return e


def graph_tile_sizes():
    """(nodes per chunk of a reduction, edges per chunk of the linearisation) of rr_graph.hip"""
    a, b = C.c_int(0), C.c_int(0)
    lib().rr_graph_tile_sizes(C.byref(a), C.byref(b))
    return a.value, b.value


def _graph_edges_arg(edges):
    e = np.asarray(edges)
    if e.dtype != GRAPH_EDGE_DTYPE or e.ndim != 1:
        raise ValueError("edges must be a one-dimensional GRAPH_EDGE_DTYPE array (native.graph_edges makes one)")
    return np.ascontiguousarray(e)


def _graph_shape(n_nodes, n_edges):
    return _int_in(n_nodes, 1, GRAPH_MAX_NODES, "n_nodes"), _int_in(n_edges, 0, GRAPH_MAX_EDGES, "n_edges")


# rr_default_detect_config
DETECT_DEFAULTS ={"method": 0, "guard_cells": 2, "train_cells": 16, "k": 12, "min_intensity": 1, "min_bin": 0, "cfar_scale": 3.0}
DETECT_METHODS = {"cfar": 0, "ca-cfar": 0, "kstrongest": 1, "k-strongest": 1, 0: 0, 1: 1}

# rr_default_window_detect_config
WINDOW_DEFAULTS = {"method": 3, "guard_range": 2, "train_range": 16, "guard_azimuth": 1, "train_azimuth": 2, "rank_permille": 750,
                   "min_intensity": 1, "min_bin": 0, "scale": 3.0}
WINDOW_METHODS = {"ca": 0, "go": 1, "so": 2, "os": 3, 0: 0, 1: 1, 2: 2, 3: 3}
WINDOW_MAX_CELLS = 65535


# rr_image_metrics as numpy sees it (72 B), and the RR_METRIC_* bits of `which`
METRICS_DTYPE = np.dtype([("psnr", "<f8"), ("sse", "<u8"), ("ssim", "<f8"), ("hx", "<f8"), ("hy", "<f8"), ("hxy", "<f8"),
                          ("mi", "<f8"), ("nmi", "<f8"), ("voi", "<f8")])
RRImageMetrics = np.ctypeslib.as_ctypes_type(METRICS_DTYPE)
METRIC_PSNR, METRIC_SSIM, METRIC_INFO = 1, 2, 4
METRIC_ALL = METRIC_PSNR | METRIC_SSIM | METRIC_INFO
METRIC_NAMES = {"psnr": METRIC_PSNR, "ssim": METRIC_SSIM, "info": METRIC_INFO}

# rr_align_record as numpy sees it (72 B)
ALIGN_DTYPE = np.dtype([("shift", "<i4"), ("n_best", "<i4"), ("xcorr", "<i8"), ("sse", "<u8"), ("psnr", "<f8"), ("ncc", "<f8"),
                        ("sum_x", "<u8"), ("sum_xx", "<u8"), ("sum_r", "<u8"), ("sum_rr", "<u8")])
RRAlignRecord = np.ctypeslib.as_ctypes_type(ALIGN_DTYPE)

# rr_shift_record as numpy sees it (128 B)
SHIFT_DTYPE = np.dtype([("dy", "<i4"), ("dx", "<i4"), ("n_best", "<i4"), ("reserved_", "<i4"), ("xcorr", "<i8"), ("sse", "<u8"),
                        ("psnr", "<f8"), ("ncc", "<f8"), ("sub_dy", "<f8"), ("sub_dx", "<f8"), ("sse_nb", "<u8", (4,)),
                        ("sum_x", "<u8"), ("sum_xx", "<u8"), ("sum_r", "<u8"), ("sum_rr", "<u8")])
RRShiftRecord = np.ctypeslib.as_ctypes_type(SHIFT_DTYPE)


class RRPlaceConfig(C.Structure):
    _fields_ = [("cell_begin", C.c_int32), ("cell_end", C.c_int32), ("n_rings", C.c_int32), ("n_sectors", C.c_int32)]


# rr_place_match as numpy sees it (40 B)
PLACE_DTYPE = np.dtype([("index", "<u4"), ("shift", "<i4"), ("sse", "<u4"), ("n_best", "<u4"), ("xcorr", "<i8"), ("ncc", "<f8"), ("psnr", "<f8")])
RRPlaceMatch = np.ctypeslib.as_ctypes_type(PLACE_DTYPE)


def metrics_mask(which):
    """RR_METRIC_* mask from an int, a name ("psnr", "ssim", "info") or an iterable of names; ValueError otherwise"""
    if isinstance(which, str):
        which = [which]
    if isinstance(which, (int, np.integer)) and not isinstance(which, bool):
        m = int(which)
    else:
        try:
            m = 0
            for w in which:
                m |= METRIC_NAMES[w]
        except (TypeError, KeyError):
            raise ValueError("metrics must be a mask of METRIC_PSNR | METRIC_SSIM | METRIC_INFO or names from %s, got %r" % (sorted(METRIC_NAMES), which))
    if m <= 0 or m & ~METRIC_ALL:
        raise ValueError("metrics must be a non-empty mask of METRIC_PSNR | METRIC_SSIM | METRIC_INFO, got %r" % (which,))
    return m


def _win_arg(which, win_size):
    if which & METRIC_SSIM and (isinstance(win_size, bool) or not isinstance(win_size, (int, np.integer)) or not 3 <= win_size <= 15 or win_size % 2 == 0):
        raise ValueError("win_size must be an odd integer in 3..15, got %r" % (win_size,))
    return int(win_size)


def entropies_from_counts(H):
    """hx, hy, hxy, mi, nmi, voi (nats, the definitions of include/radarays_mi355.h) of a 2-D array of joint counts"""
    H = np.asarray(H, np.float64)
    n = H.sum()

    def ent(c):
        c = c[c > 0]
        return float(np.sum(c * (np.log(n) - np.log(c))) / n)
    hx, hy, hxy = ent(H.sum(1)), ent(H.sum(0)), ent(H.ravel())
    return {"hx": hx, "hy": hy, "hxy": hxy, "mi": hx + hy - hxy, "nmi": 1.0 if hxy == 0.0 else (hx + hy) / hxy, "voi": 2.0 * hxy - hx - hy}


def metrics_from_joint_histogram(H, bins=256):
    """The information metrics from one exact joint histogram (uint32 [256][256], H[a][b] = pixels with image value a and
    reference value b) without a second pass over the images.  bins = 256: one bin per grey level, what the library's
    record holds.  Fewer bins (skimage's normalized_mutual_information defaults to 100): the counts are regrouped by numpy's
    histogram rule -- per image, `bins` equal-width bins over its own min..max (read off the non-empty marginals; a constant
    image gets min - 0.5 .. max + 0.5), a value on an inner edge goes to the bin on its right, the maximum to the last bin."""
    H = np.asarray(H)
    if H.shape != (256, 256):
        raise ValueError("joint histogram must be [256][256], got %s" % (H.shape,))
    bins = _int_in(bins, 1, 256, "bins")
    if H.sum() == 0:
        raise ValueError("empty joint histogram")
    if bins == 256:
        return entropies_from_counts(H)
    idx = []
    for marg in (H.sum(1), H.sum(0)):
        used = np.nonzero(marg)[0]
        lo, hi = float(used[0]), float(used[-1])
        if lo == hi:
            lo, hi = lo - 0.5, hi + 0.5
        edges = np.linspace(lo, hi, bins + 1)
        g = np.arange(256, dtype=np.float64)
        i = np.searchsorted(edges, g, side="right") - 1
        i[g == edges[-1]] = bins - 1
        idx.append(np.clip(i, 0, bins - 1))          # (levels outside min..max hold no pixels)
    B = np.zeros((bins, bins), np.int64)
    np.add.at(B, (idx[0][:, None], idx[1][None, :]), H.astype(np.int64))
    return entropies_from_counts(B)


class RRStats(C.Structure):
    _fields_ = [("wave_passes", C.c_uint64), ("hits", C.c_uint64), ("signals", C.c_uint64),
                ("nodes_visited", C.c_uint64), ("tris_tested", C.c_uint64),
                ("overflow", C.c_uint32), ("pad_", C.c_uint32)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad_"}


# every struct include/radarays_mi355.h gives a body -> (its ctypes Structure, its numpy dtype or None).  tests/test_abi.py holds each to
# the header's field list and to gcc's sizeof / offsetof.
STRUCTS = {
    "rr_material": (RRMaterial, None), "rr_config": (RRConfig, None), "rr_stats": (RRStats, None), "rr_param_set": (RRParamSet, None),
    "rr_image_metrics": (RRImageMetrics, METRICS_DTYPE), "rr_align_record": (RRAlignRecord, ALIGN_DTYPE),
    "rr_echo": (np.ctypeslib.as_ctypes_type(ECHO_DTYPE), ECHO_DTYPE), "rr_echo_src": (np.ctypeslib.as_ctypes_type(ECHO_SRC_DTYPE), ECHO_SRC_DTYPE),
    "rr_wave_rec": (RRWaveRec, WAVE_DTYPE), "rr_detect_config": (RRDetectConfig, None), "rr_radar_point": (RRRadarPoint, POINT_DTYPE),
    "rr_window_detect_config": (RRWindowDetectConfig, None),
    "rr_cartesian_config": (RRCartesianConfig, None), "rr_object_note": (RRObjectNote, NOTE_DTYPE), "rr_shift_record": (RRShiftRecord, SHIFT_DTYPE),
    "rr_place_config": (RRPlaceConfig, None), "rr_place_match": (RRPlaceMatch, PLACE_DTYPE), "rr_sweep_rec": (RRSweepRec, SWEEP_DTYPE),
    "rr_icp_rec": (RRIcpRec, ICP_DTYPE), "rr_field_config": (RRFieldConfig, None), "rr_field_rec": (RRFieldRec, FIELD_DTYPE),
    "rr_occupancy_config": (RROccupancyConfig, None), "rr_filter_config": (RRFilterConfig, FILTER_CONFIG_DTYPE),
    "rr_filter_summary": (RRFilterSummary, FILTER_SUMMARY_DTYPE), "rr_mesh": (RRMesh, None),
    "rr_beam_config": (RRBeamConfig, None), "rr_beam_rec": (RRBeamRec, BEAM_DTYPE), "rr_slice_config": (RRSliceConfig, None),
    "rr_components_config": (RRComponentsConfig, None), "rr_component": (RRComponent, COMPONENT_DTYPE),
    "rr_corr_config": (RRCorrConfig, None), "rr_corr_rec": (RRCorrRec, CORR_DTYPE),
    "rr_surfel_config": (RRSurfelConfig, None), "rr_surfel": (RRSurfel, SURFEL_DTYPE),
    "rr_graph_edge": (RRGraphEdge, GRAPH_EDGE_DTYPE), "rr_graph_config": (RRGraphConfig, None), "rr_graph_rec": (RRGraphRec, GRAPH_REC_DTYPE),
}


def _prototypes():
    """the one table of entry points: name -> (return type, argument types), in the header's order.  A new entry point is one row here;
    tests/test_abi.py compares every row with the header's prototype, and the header with this table."""
    P, vp, i, sz, f, s = C.POINTER, C.c_void_p, C.c_int, C.c_size_t, C.c_float, C.c_char_p
    i32, u32, u64, u, dbl = C.c_int32, C.c_uint32, C.c_uint64, C.c_uint, C.c_double
    return {
        # ---- context, scene, frames
        "rr_default_config": (None, [P(RRConfig)]),
        "rr_create": (vp, [i]),
        "rr_destroy": (None, [vp]),
        "rr_last_error": (s, [vp]),
        "rr_abi_version": (i, []),
        "rr_set_mesh": (i, [vp, vp, sz, vp, sz, vp]),
        "rr_set_mesh_gpu": (i, [vp, vp, sz, vp, sz, vp]),
        "rr_copy_mesh": (i, [vp, vp]),
        "rr_set_object_poses": (i, [vp, vp, sz]),
        "rr_update_vertices": (i, [vp, vp, sz]),
        "rr_set_object_twists": (i, [vp, vp, sz]),
        "rr_get_tree_cost": (i, [vp, P(dbl), P(dbl)]),
        "rr_rebuild_tree": (i, [vp, i]),
        "rr_set_materials": (i, [vp, vp, sz, vp, sz, i32]),
        "rr_set_config": (i, [vp, P(RRConfig)]),
        "rr_set_beam_samples": (i, [vp, vp, sz]),
        "rr_set_noise_offsets": (i, [vp, vp, sz]),
        "rr_set_motion_poses": (i, [vp, vp, sz]),
        "rr_simulate": (i, [vp, vp, i, i, vp, vp, P(RRStats)]),
        "rr_simulate_columns_device": (i, [vp, vp, i, i, vp, vp, vp]),
        "rr_simulate_batch_columns_device": (i, [vp, vp, i, i, i, vp, vp]),
        "rr_simulate_batch_device": (i, [vp, vp, i, vp, vp]),
        "rr_simulate_batch_host_async": (i, [vp, vp, i, vp, vp]),
        "rr_wait_host": (i, [vp, vp]),
        "rr_host_alloc": (vp, [sz]),
        "rr_host_free": (None, [vp]),
        "rr_copy_to_host_async": (i, [vp, vp, vp, sz, vp]),
        "rr_deliver_to_host_async": (i, [vp, vp, vp, sz, vp]),
        "rr_host_delivery_route": (i, [vp]),
        "rr_assemble_image_device": (i, [vp, vp, vp, vp]),
        "rr_assemble_blocks_device": (i, [vp, vp, i, sz, vp, vp]),
        "rr_simulate_material_sets_device": (i, [vp, vp, vp, i, sz, vp, vp]),
        "rr_simulate_material_sets": (i, [vp, vp, vp, i, sz, vp]),
        "rr_simulate_param_sets_device": (i, [vp, vp, P(RRParamSet), i, sz, vp, vp]),
        "rr_score_images_device": (i, [vp, vp, i, vp, vp, vp, vp]),
        "rr_simulate_param_sets": (i, [vp, vp, P(RRParamSet), i, sz, vp, vp, vp]),
        # ---- image metrics (rr_metrics.hip)
        "rr_compare_images_device": (i, [vp, vp, i, vp, u32, i, vp, vp, vp]),
        "rr_compare_images": (i, [vp, vp, i, vp, u32, i, vp, vp]),
        "rr_simulate_param_sets_metrics": (i, [vp, vp, P(RRParamSet), i, sz, vp, vp, u32, i, vp]),
        # ---- azimuth registration (rr_align.hip)
        "rr_align_images_device": (i, [vp, vp, i, vp, i, i, vp, vp, vp]),
        "rr_align_images": (i, [vp, vp, i, vp, i, i, vp, vp]),
        "rr_simulate_batch_align": (i, [vp, vp, i, vp, i, i, vp, vp, vp]),
        # ---- frames assembled from blocks, streams, statistics
        "rr_assemble_frames_device": (i, [vp, vp, i, sz, i, sz, vp, vp]),
        "rr_simulate_device": (i, [vp, vp, vp, vp]),
        "rr_synchronize": (i, [vp, vp]),
        "rr_peek_error_bits_async": (i, [vp, vp, vp]),
        "rr_get_stats": (i, [vp, P(RRStats)]),
        "rr_set_stats_mode": (i, [vp, i]),
        "rr_get_traversal_shape": (i, [vp, vp]),
        # ---- introspection used by tests / bench
        "rr_debug_trace": (i, [vp, vp, vp, sz, vp, vp]),
        "rr_debug_fresnel": (i, [vp, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "rr_debug_brdf": (i, [vp, sz, vp, i, vp]),
        "rr_debug_column": (i, [vp, i, i, i, i, i, i, vp, vp, sz, vp, vp, vp, sz, vp, vp, vp]),
        "rr_get_bvh_info": (i, [vp, P(u64), P(u64), P(u32), P(u32)]),
        "rr_get_trace_grid": (i, [vp, vp, vp, P(u64)]),
        "rr_get_graph_stats": (i, [vp, P(u64), P(u64)]),
        "rr_set_timing_mode": (i, [vp, i]),
        "rr_get_kernel_time": (i, [vp, s, P(dbl), P(u64), i]),
        "rr_get_kernel_samples": (i, [vp, s, vp, sz, P(sz)]),
        "rr_reserve_timing_events": (i, [vp, sz]),
        # ---- echo provenance (rr_labels.hip)
        "rr_simulate_batch_provenance_device": (i, [vp, vp, i, vp, vp, vp, vp, sz, vp, vp]),
        "rr_simulate_provenance": (i, [vp, vp, vp, vp, vp, vp, sz, vp]),
        "rr_debug_labels": (i, [vp, i, i, vp, vp, sz, vp, vp]),
        # ---- wave paths (rr_paths.hip)
        "rr_simulate_batch_paths_device": (i, [vp, vp, i, vp, vp, sz, vp, vp, u, vp]),
        "rr_simulate_paths": (i, [vp, vp, vp, vp, sz, vp, vp, u]),
        # ---- Doppler (rr_doppler.hip)
        "rr_simulate_batch_doppler_device": (i, [vp, vp, i, vp, f, vp, vp, sz, vp, vp, vp, vp]),
        "rr_simulate_doppler": (i, [vp, vp, vp, f, vp, vp, vp, sz, vp, vp, vp]),
        # ---- point clouds and Cartesian images (rr_detect.hip)
        "rr_default_detect_config": (None, [P(RRDetectConfig)]),
        "rr_detect_device": (i, [vp, vp, i, P(RRDetectConfig), vp, i, vp, vp]),
        "rr_detect": (i, [vp, vp, i, P(RRDetectConfig), vp, i, vp]),
        "rr_default_window_detect_config": (None, [P(RRWindowDetectConfig)]),
        "rr_detect_window_device": (i, [vp, vp, i, P(RRWindowDetectConfig), vp, i, vp, vp, vp]),
        "rr_detect_window": (i, [vp, vp, i, P(RRWindowDetectConfig), vp, i, vp, vp]),
        "rr_detect_window_tile_sizes": (i, [P(RRWindowDetectConfig), i, i, P(i)]),
        "rr_polar_to_cartesian_device": (i, [vp, vp, i, P(RRCartesianConfig), vp, vp]),
        "rr_polar_to_cartesian": (i, [vp, vp, i, P(RRCartesianConfig), vp]),
        # ---- object annotations (rr_notes.hip)
        "rr_annotate_scratch_bytes": (sz, [i, i, i]),
        "rr_annotate_labels_device": (i, [vp, vp, vp, i, i, u32, vp, vp, vp, sz, vp]),
        "rr_annotate_labels": (i, [vp, vp, vp, i, i, u32, vp, vp]),
        "rr_label_points_device": (i, [vp, vp, vp, i, i, vp, vp, vp, vp, vp, vp, vp]),
        "rr_polar_to_cartesian_labels_device": (i, [vp, vp, i, P(RRCartesianConfig), vp, vp]),
        "rr_polar_to_cartesian_labels": (i, [vp, vp, i, P(RRCartesianConfig), vp]),
        "rr_simulate_batch_annotations": (i, [vp, vp, i, u32, vp, vp, vp]),
        # ---- translation registration (rr_shift.hip)
        "rr_shift_images_device": (i, [vp, vp, i, vp, i, i, i, vp, vp, vp, vp]),
        "rr_shift_images": (i, [vp, vp, i, vp, i, i, i, vp, vp, vp]),
        "rr_simulate_batch_shift": (i, [vp, vp, i, vp, P(RRCartesianConfig), i, vp, vp, vp]),
        # ---- place recognition (rr_place.hip)
        "rr_describe_images_device": (i, [vp, vp, i, P(RRPlaceConfig), vp, vp]),
        "rr_describe_images": (i, [vp, vp, i, P(RRPlaceConfig), vp]),
        "rr_simulate_batch_describe": (i, [vp, vp, i, P(RRPlaceConfig), vp]),
        "rr_match_descriptors_device": (i, [vp, vp, i, vp, i, i, i, i, vp, vp, vp, vp]),
        "rr_match_descriptors": (i, [vp, vp, i, vp, i, i, i, i, vp, vp, vp]),
        # ---- sweep compensation (rr_deskew.hip)
        "rr_sweep_table_device": (i, [vp, vp, vp, vp, f, i, vp, vp]),
        "rr_sweep_table": (i, [vp, vp, vp, vp, f, i, vp]),
        "rr_compensate_points_device": (i, [vp, vp, vp, i, i, vp, vp, vp]),
        "rr_compensate_points": (i, [vp, vp, vp, i, i, vp, vp]),
        "rr_polar_to_cartesian_sweep_device": (i, [vp, vp, i, P(RRCartesianConfig), vp, i, vp, vp]),
        "rr_polar_to_cartesian_sweep": (i, [vp, vp, i, P(RRCartesianConfig), vp, i, vp]),
        # ---- scan matching (rr_icp.hip)
        "rr_register_points_device": (i, [vp, vp, vp, i, i, vp, vp, i, vp, f, i, vp, vp, vp]),
        "rr_register_points": (i, [vp, vp, vp, i, i, vp, u32, i, vp, f, i, vp, vp]),
        "rr_icp_tile_sizes": (None, [P(i), P(i)]),
        # ---- likelihood field (rr_field.hip)
        "rr_rasterize_points_device": (i, [vp, vp, vp, i, i, vp, P(RRFieldConfig), vp, vp]),
        "rr_rasterize_points": (i, [vp, vp, vp, i, i, vp, P(RRFieldConfig), vp]),
        "rr_distance_field_device": (i, [vp, vp, i, P(RRFieldConfig), vp, vp]),
        "rr_distance_field": (i, [vp, vp, i, P(RRFieldConfig), vp]),
        "rr_score_poses_device": (i, [vp, vp, vp, i, vp, i, vp, P(RRFieldConfig), vp, vp]),
        "rr_score_poses": (i, [vp, vp, u32, i, vp, i, vp, P(RRFieldConfig), vp]),
        "rr_field_tile_sizes": (None, [P(i), P(i), P(i)]),
        # ---- occupancy mapping (rr_occupancy.hip)
        "rr_occupancy_update_device": (i, [vp, vp, vp, i, i, vp, P(RRFieldConfig), P(RROccupancyConfig), vp, vp, vp]),
        "rr_occupancy_update": (i, [vp, vp, vp, i, i, vp, P(RRFieldConfig), P(RROccupancyConfig), vp]),
        "rr_occupancy_map_device": (i, [vp, vp, P(RRFieldConfig), vp, vp]),
        "rr_occupancy_map": (i, [vp, vp, P(RRFieldConfig), vp]),
        "rr_occupancy_tile_sizes": (None, [P(i), P(i), P(i)]),
        # ---- particle filter step (rr_filter.hip)
        "rr_filter_resample_device": (i, [vp, vp, i, vp, i, P(RRFilterConfig), vp, vp, vp, vp]),
        "rr_filter_resample": (i, [vp, vp, i, vp, i, P(RRFilterConfig), vp, vp, vp]),
        "rr_filter_move_device": (i, [vp, vp, i, vp, i, f, f, f, f, P(RRFilterConfig), vp, vp]),
        "rr_filter_move": (i, [vp, vp, i, vp, i, f, f, f, f, P(RRFilterConfig), vp]),
        "rr_filter_tile_sizes": (None, [P(i), P(i), P(i)]),
        # ---- map refinement (rr_refine.hip)
        "rr_nearest_field_device": (i, [vp, vp, i, P(RRFieldConfig), vp, vp]),
        "rr_nearest_field": (i, [vp, vp, i, P(RRFieldConfig), vp]),
        "rr_refine_poses_device": (i, [vp, vp, vp, i, vp, i, vp, P(RRFieldConfig), i, vp, vp]),
        "rr_refine_poses": (i, [vp, vp, u32, i, vp, i, vp, P(RRFieldConfig), i, vp]),
        "rr_refine_tile_sizes": (None, [P(i), P(i), P(i)]),
        # ---- beam model (rr_cast.hip)
        "rr_scan_profile_device": (i, [vp, vp, vp, i, i, vp, vp]),
        "rr_scan_profile": (i, [vp, vp, vp, i, i, vp]),
        "rr_cast_map_device": (i, [vp, vp, i, vp, vp, P(RRFieldConfig), P(RRBeamConfig), vp, vp]),
        "rr_cast_map": (i, [vp, vp, i, vp, vp, P(RRFieldConfig), P(RRBeamConfig), vp]),
        "rr_score_beams_device": (i, [vp, vp, vp, i, vp, vp, P(RRFieldConfig), P(RRBeamConfig), vp, vp]),
        "rr_score_beams": (i, [vp, vp, vp, i, vp, vp, P(RRFieldConfig), P(RRBeamConfig), vp]),
        "rr_cast_tile_sizes": (None, [P(i), P(i), P(i)]),
        # ---- mesh maps (rr_slice.hip)
        "rr_slice_mesh_device": (i, [vp, P(RRSliceConfig), P(RRFieldConfig), vp, vp, vp, vp]),
        "rr_slice_mesh": (i, [vp, P(RRSliceConfig), P(RRFieldConfig), vp, vp, vp]),
        "rr_slice_tile_sizes": (None, [P(i), P(i), P(i)]),
        # ---- connected components (rr_components.hip)
        "rr_components_scratch_bytes": (sz, [i, P(RRComponentsConfig)]),
        "rr_components_tile_sizes": (None, [P(i), P(i)]),
        "rr_label_components_device": (i, [vp, vp, i, P(RRComponentsConfig), vp, vp, vp, vp, vp, sz, vp]),
        "rr_label_components": (i, [vp, vp, i, P(RRComponentsConfig), vp, vp, vp, vp]),
        # ---- correlative scan matching (rr_correlate.hip)
        "rr_correlate_scratch_bytes": (sz, [i, i, P(RRCorrConfig)]),
        "rr_correlate_tile_sizes": (None, [P(i), P(i), P(i)]),
        "rr_field_pyramid_device": (i, [vp, vp, P(RRFieldConfig), i, vp, vp]),
        "rr_field_pyramid": (i, [vp, vp, P(RRFieldConfig), i, vp]),
        "rr_correlate_scan_device": (i, [vp, vp, vp, i, vp, i, vp, P(RRFieldConfig), P(RRCorrConfig), vp, vp, sz, vp]),
        "rr_correlate_scan": (i, [vp, vp, u32, i, vp, i, vp, P(RRFieldConfig), P(RRCorrConfig), vp]),
        # ---- oriented surface points and point-to-line scan matching (rr_surfels.hip)
        "rr_surfels_scratch_bytes": (sz, [i, P(RRSurfelConfig)]),
        "rr_surfels_tile_sizes": (None, [P(i), P(i)]),
        "rr_surface_points_device": (i, [vp, vp, vp, i, i, P(RRSurfelConfig), vp, i, vp, vp, sz, vp]),
        "rr_surface_points": (i, [vp, vp, vp, i, i, P(RRSurfelConfig), vp, i, vp]),
        "rr_register_surfels_device": (i, [vp, vp, vp, i, i, vp, vp, i, vp, f, i, vp, vp, vp]),
        "rr_register_surfels": (i, [vp, vp, vp, i, i, vp, u32, i, vp, f, i, vp, vp]),
        # ---- pose-graph optimisation (rr_graph.hip)
        "rr_graph_tile_sizes": (None, [P(i), P(i)]),
        "rr_graph_plan_bytes": (sz, [i, i]),
        "rr_graph_scratch_bytes": (sz, [i, i, P(RRGraphConfig)]),
        "rr_graph_plan_device": (i, [vp, vp, i, i, vp, sz, vp]),
        "rr_graph_plan": (i, [vp, vp, i, i, vp, sz]),
        "rr_optimize_graph_device": (i, [vp, vp, vp, vp, i, i, vp, P(RRGraphConfig), vp, vp, vp, sz, vp]),
        "rr_optimize_graph": (i, [vp, vp, vp, vp, i, i, vp, P(RRGraphConfig), vp, vp]),
        # ---- several GPUs of one node behind one object (rr_multi.hip)
        "rr_create_multi": (vp, [P(i), i]),
        "rr_destroy_multi": (None, [vp]),
        "rr_multi_last_error": (s, [vp]),
        "rr_multi_device_count": (i, [vp]),
        "rr_multi_rccl_version": (i, [vp]),
        "rr_multi_ctx": (vp, [vp, i]),
        "rr_partition": (None, [i, i, i, P(i), P(i)]),
        "rr_multi_plan": (i, [i, i, i, i, P(i), P(sz), vp, vp, vp]),
        "rr_multi_set_mesh": (i, [vp, vp, sz, vp, sz, vp]),
        "rr_multi_set_mesh_gpu": (i, [vp, vp, sz, vp, sz, vp]),
        "rr_multi_set_object_poses": (i, [vp, vp, sz]),
        "rr_multi_update_vertices": (i, [vp, vp, sz]),
        "rr_multi_rebuild_tree": (i, [vp, i]),
        "rr_multi_set_materials": (i, [vp, vp, sz, vp, sz, i32]),
        "rr_multi_set_config": (i, [vp, P(RRConfig)]),
        "rr_multi_set_beam_samples": (i, [vp, vp, sz]),
        "rr_multi_set_noise_offsets": (i, [vp, vp, sz]),
        "rr_multi_set_motion_poses": (i, [vp, vp, sz]),
        "rr_multi_simulate": (i, [vp, vp, vp]),
        "rr_multi_simulate_batch": (i, [vp, vp, i, vp]),
        "rr_multi_simulate_batch_async": (i, [vp, vp, i, vp]),
        "rr_multi_wait": (i, [vp, vp]),
        # ---- host side of the seam (no GPU involved)
        "rr_cone_dirs": (i, [f, i, f, vp, vp, sz, vp]),
        "rr_sample_cone_local": (i, [u32, f, sz, i, f, vp]),
        "rr_load_mesh_file": (i, [s, P(RRMesh), s, sz]),
        "rr_mesh_reorder_objects": (i, [P(RRMesh), P(s), sz, s, sz]),
        "rr_free_mesh": (None, [P(RRMesh)]),
    }


PROTOTYPES = _prototypes()
SYMBOLS = list(PROTOTYPES)


def build(force=False):
    """hipcc --offload-arch=gfx950 build of the in-tree shared library."""
    src = os.path.join(_HERE, "csrc")
    srcs = [os.path.join(src, f) for f in os.listdir(src)] + [os.path.join(_HERE, "..", "include", "radarays_mi355.h")]
    stale = (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(f) > os.path.getmtime(LIB_PATH) for f in srcs)
    if force or stale:
        subprocess.run(["make", "-C", src], check=True, stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "radarays_ros_amd: %s is missing -- build it with __graft_entry__.build() "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    try:
        # share torch's HIP runtime when torch is in the process: both resolve the
        # SONAME libamdhip64.so.7, the first one loaded wins
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)          # AttributeError: the library lacks an entry point the header declares
        fn.restype, fn.argtypes = restype, argtypes
    _LIB = L
    return L


def _ptr(a):
    """an optional array -> its address, or None (a null pointer)"""
    return None if a is None else a.ctypes.data


def _rows(a, width, what):
    """a numeric array of shape [n][width] (or flat, n * width values) -> contiguous float32 [n][width]; ValueError otherwise"""
    x = np.asarray(a)
    if x.dtype.kind not in "fiu":
        raise ValueError("%s must be real numbers, got dtype %s" % (what, x.dtype))
    if not ((x.ndim == 2 and x.shape[1] == width) or (x.ndim == 1 and x.size % width == 0)):
        raise ValueError("%s must have shape [n][%d], got %s" % (what, width, x.shape))
    return np.ascontiguousarray(x, np.float32).reshape(-1, width)


def _pose_batch(poses):
    """the poses of one batched call: float32 [n][7], n in 1..64 (RR_MAX_BATCH)"""
    p = _rows(poses, 7, "poses")
    if not 1 <= len(p) <= 64:
        raise ValueError("1..64 poses, got %d" % len(p))
    return p


_A_CLOUD = "one-dimensional POINT_DTYPE array"      # the words every refusal of a cloud shares


def _scan(points, lo, what):
    """one POINT_DTYPE cloud -> contiguous.  lo 0 or 1: it holds lo..ICP_MAX_POINTS points; lo None: its length is the caller's to check"""
    p = np.asarray(points)
    if p.dtype != POINT_DTYPE or p.ndim != 1 or (lo is not None and not lo <= len(p) <= ICP_MAX_POINTS):
        span = "" if lo is None else (" of at most %d points", " of 1..%d points")[lo] % ICP_MAX_POINTS
        raise ValueError("%s must be a %s%s" % (what, _A_CLOUD, span))
    return np.ascontiguousarray(p)


def _states(states, dtype, what, n_max=None, n=None):
    """real numbers [n][4] = (c, s, tx, ty) -> contiguous `dtype`; n is in 1..n_max, or exactly the `n` given"""
    x = np.asarray(states)
    if n is None:
        fits, rows = x.ndim == 2 and x.shape[1] == 4 and 1 <= len(x) <= n_max, "[n][4] (c, s, tx, ty), n in 1..%d" % n_max
    else:
        fits, rows = x.shape == (n, 4), "[%d][4] (c, s, tx, ty)" % n
    if x.dtype.kind not in "fiu" or not fits:
        raise ValueError("%s must be real numbers of shape %s, got %s %s" % (what, rows, x.dtype, x.shape))
    return np.ascontiguousarray(x, dtype)


def _cloud_list(points):
    """1..65535 POINT_DTYPE arrays in a list (or one such array) -> the list.  The first step of _clouds"""
    if isinstance(points, np.ndarray) and points.ndim == 1:
        points = [points]
    pts = [np.asarray(p) for p in points]
    if not pts or len(pts) > 65535 or any(p.dtype != POINT_DTYPE or p.ndim != 1 for p in pts):
        raise ValueError("points must be a list of 1..65535 %ss" % _A_CLOUD)
    return pts


def _cloud_offsets(offsets, n, n_angles):
    """uint32 [n][n_angles + 1] (or one frame's [n_angles + 1]) -> contiguous and two-dimensional.  The second step of _clouds"""
    offs = np.asarray(offsets)
    if offs.ndim == 1:
        offs = offs[None]
    if offs.dtype != np.uint32 or offs.shape != (n, n_angles + 1):
        raise ValueError("offsets must be uint32 [%d][%d], got %s %s" % (n, n_angles + 1, offs.dtype, offs.shape))
    return np.ascontiguousarray(offs)


def _clouds(points, offsets, n_angles, cap):
    """what detect() (or compensate_points()) returned, a list of n POINT_DTYPE arrays and offsets uint32 [n][n_angles + 1] -> (the points
    as one zero-padded POINT_DTYPE [n][max_points] block, the contiguous offsets, the n lengths).  cap: a cloud holds at most ICP_MAX_POINTS
    points.  Refused in this order: the list, the cap, the offsets, a frame that does not hold the points its offsets count.  A caller
    with a check of its own between two of these takes the steps before it by themselves (_cloud_list, _cloud_offsets) and hands their
    results in here, where they pass again: of two faults it then reports the one it always has."""
    pts = _cloud_list(points)
    lens = [len(p) for p in pts]
    if cap and max(lens) > ICP_MAX_POINTS:
        raise ValueError("a cloud may hold at most %d points" % ICP_MAX_POINTS)
    offs = _cloud_offsets(offsets, len(pts), n_angles)
    mp = max(1, max(lens))
    if any(k != min(int(offs[f, -1]), mp) for f, k in enumerate(lens)):
        raise ValueError("every frame must hold the points its offsets count")
    buf = np.zeros((len(pts), mp), POINT_DTYPE)
    for f, p in enumerate(pts):
        buf[f, :len(p)] = p
    return buf, offs, lens


def object_poses_array(poses):
    """[n_objects][7] (qx qy qz qw tx ty tz) -> float32, shape-checked before any call into the library"""
    return _rows(poses, 7, "object poses")


def vertex_array(verts):
    """[nv][3] -> float32, shape-checked before any call into the library"""
    return _rows(verts, 3, "vertices")


def builder_id(builder):
    b = {"host": 0, "gpu": 1, 0: 0, 1: 1}.get(builder) if isinstance(builder, (str, int)) else None
    if b is None:
        raise ValueError("builder must be 'host' or 'gpu', got %r" % (builder,))
    return b


def make_config(cfg, n_angles=400, max_waves_per_azimuth=0, wave_energy_threshold=0.001,
                ray_range_max=1000.0, brdf_model=0, theta_min=0.0, theta_inc=None):
    """RadarModelConfig (params.py) -> rr_config.  theta_inc None: the reference's clockwise sweep, -2 pi / n_angles."""
    c = RRConfig()
    lib().rr_default_config(C.byref(c))
    c.n_cells = int(cfg.n_cells)
    c.n_angles = int(n_angles)
    c.n_reflections = int(cfg.n_reflections)
    c.signal_denoising = int(cfg.signal_denoising)
    c.signal_denoising_triangular_width = int(cfg.signal_denoising_triangular_width)
    c.signal_denoising_gaussian_width = int(cfg.signal_denoising_gaussian_width)
    c.signal_denoising_mb_width = int(cfg.signal_denoising_mb_width)
    c.ambient_noise = int(cfg.ambient_noise)
    c.scroll_image = int(cfg.scroll_image)
    c.record_multi_reflection = int(bool(cfg.record_multi_reflection))
    c.record_multi_path = int(bool(cfg.record_multi_path))
    c.max_waves_per_azimuth = int(max_waves_per_azimuth)
    c.brdf_model = int(brdf_model)
    for k in ("resolution", "energy_max", "signal_max", "signal_denoising_triangular_mode",
              "signal_denoising_gaussian_mode", "signal_denoising_mb_mode",
              "ambient_noise_at_signal_0", "ambient_noise_at_signal_1",
              "ambient_noise_energy_max", "ambient_noise_energy_min",
              "ambient_noise_energy_loss", "multipath_threshold"):
        setattr(c, k, float(getattr(cfg, k)))
    c.wave_energy_threshold = float(np.float32(wave_energy_threshold))
    c.theta_min = float(np.float32(theta_min))
    c.theta_inc = float(np.float32(-(2.0 * np.pi) / n_angles if theta_inc is None else theta_inc))   # Radar.cpp:27
    c.range_max = float(ray_range_max)                            # radar_algorithms.cpp:158
    return c


class RRError(RuntimeError):
    pass


def _int_in(v, lo, hi, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError("%s must be an integer in [%d, %d], got %r" % (what, lo, hi, v))
    return int(v)


def detect_config(cfg=None, n_cells=None, **kw):
    """RRDetectConfig from an RRDetectConfig, a dict and/or keywords over DETECT_DEFAULTS; every field is range-checked here
    (k and min_bin against n_cells when it is given), before any call into the library.  method: 0 / "cfar", 1 / "kstrongest"."""
    d = dict(DETECT_DEFAULTS)
    if isinstance(cfg, RRDetectConfig):
        d.update({k: getattr(cfg, k) for k in DETECT_DEFAULTS})
    elif isinstance(cfg, dict):
        d.update(cfg)
    elif cfg is not None:
        raise ValueError("detection config must be an RRDetectConfig or a dict, got %r" % (cfg,))
    d.update(kw)
    unknown = set(d) - set(DETECT_DEFAULTS)
    if unknown:
        raise ValueError("unknown detection config fields: %s" % sorted(unknown))
    m = DETECT_METHODS.get(d["method"]) if isinstance(d["method"], (str, int)) and not isinstance(d["method"], bool) else None
    if m is None:
        raise ValueError("method must be 0 / 'cfar' or 1 / 'kstrongest', got %r" % (d["method"],))
    top = int(n_cells) if n_cells is not None else 8192
    c = RRDetectConfig()
    c.method = m
    c.guard_cells = _int_in(d["guard_cells"], 0, 1024, "guard_cells")
    c.train_cells = _int_in(d["train_cells"], 1, 1024, "train_cells")
    c.k = _int_in(d["k"], 1, top, "k")
    c.min_intensity = _int_in(d["min_intensity"], 0, 255, "min_intensity")
    c.min_bin = _int_in(d["min_bin"], 0, top - 1, "min_bin")
    try:
        scale = float(d["cfar_scale"])
    except (TypeError, ValueError):
        raise ValueError("cfar_scale must be a number, got %r" % (d["cfar_scale"],))
    with np.errstate(over="ignore"):
        finite = bool(np.isfinite(np.float32(scale)))
    if not (finite and scale >= 0.0):
        raise ValueError("cfar_scale must be finite and >= 0, got %r" % (scale,))
    c.cfar_scale = scale
    return c


def window_detect_config(cfg=None, n_cells=None, n_angles=None, **kw):
    """RRWindowDetectConfig from an RRWindowDetectConfig, a dict and/or keywords over WINDOW_DEFAULTS; every field and every refusal of
    the header is checked here (min_bin against n_cells, the column window against n_angles, when they are given), before any call into
    the library.  method: 0 / "ca", 1 / "go", 2 / "so", 3 / "os"."""
    d = dict(WINDOW_DEFAULTS)
    if isinstance(cfg, RRWindowDetectConfig):
        if any(cfg.reserved_):
            raise ValueError("reserved_ must be 0")
        d.update({k: getattr(cfg, k) for k in WINDOW_DEFAULTS})
    elif isinstance(cfg, dict):
        d.update(cfg)
    elif cfg is not None:
        raise ValueError("window detection config must be an RRWindowDetectConfig or a dict, got %r" % (cfg,))
    d.update(kw)
    unknown = set(d) - set(WINDOW_DEFAULTS)
    if unknown:
        raise ValueError("unknown window detection config fields: %s" % sorted(unknown))
    m = d["method"].lower() if isinstance(d["method"], str) else d["method"]
    m = WINDOW_METHODS.get(m) if isinstance(m, (str, int, np.integer)) and not isinstance(m, bool) else None
    if m is None:
        raise ValueError("method must be 0 / 'ca', 1 / 'go', 2 / 'so' or 3 / 'os', got %r" % (d["method"],))
    c = RRWindowDetectConfig()
    c.method = m
    c.guard_range, c.train_range = _int_in(d["guard_range"], 0, 1024, "guard_range"), _int_in(d["train_range"], 0, 1024, "train_range")
    c.guard_azimuth, c.train_azimuth = _int_in(d["guard_azimuth"], 0, 32, "guard_azimuth"), _int_in(d["train_azimuth"], 0, 32, "train_azimuth")
    c.rank_permille = _int_in(d["rank_permille"], 1, 1000, "rank_permille")
    c.min_intensity = _int_in(d["min_intensity"], 0, 255, "min_intensity")
    c.min_bin = _int_in(d["min_bin"], 0, (int(n_cells) if n_cells is not None else 8192) - 1, "min_bin")
    try:
        scale = float(d["scale"])
    except (TypeError, ValueError):
        raise ValueError("scale must be a number, got %r" % (d["scale"],))
    with np.errstate(over="ignore"):
        finite = bool(np.isfinite(np.float32(scale)))
    if not (finite and scale >= 0.0):
        raise ValueError("scale must be finite and >= 0, got %r" % (scale,))
    c.scale = scale
    if c.train_range + c.train_azimuth == 0:
        raise ValueError("no training cells: train_range + train_azimuth is 0")
    wr, wc = 2 * (c.guard_range + c.train_range) + 1, 2 * (c.guard_azimuth + c.train_azimuth) + 1
    if n_angles is not None and wc > int(n_angles):
        raise ValueError("the column window of %d columns exceeds n_angles = %d" % (wc, n_angles))
    if wr * wc > WINDOW_MAX_CELLS:
        raise ValueError("a window of %d x %d cells holds more than %d" % (wr, wc, WINDOW_MAX_CELLS))
    if m in (1, 2) and c.train_range == 0:
        raise ValueError("GO / SO need train_range >= 1")
    return c


def detect_window_tile_sizes(cfg, n_cells, n_angles):
    """rr_detect_window_tile_sizes: (rows, columns, halo rows, halo columns) of the tile a launch uses for this config and shape"""
    n_cells, n_angles = _int_in(n_cells, 1, 2**31 - 1, "n_cells"), _int_in(n_angles, 1, 2**31 - 1, "n_angles")
    c = window_detect_config(cfg, n_cells=n_cells, n_angles=n_angles)
    out = (C.c_int * 4)()
    if lib().rr_detect_window_tile_sizes(C.byref(c), n_cells, n_angles, out) != 0:
        raise ValueError("rr_detect_window_tile_sizes refused the config")
    return tuple(out)


def cartesian_config(width, pixel_size, bilinear=True):
    """RRCartesianConfig, range-checked before any call into the library"""
    c = RRCartesianConfig()
    c.width = _int_in(width, 1, 8192, "width")
    try:
        ps = float(pixel_size)
    except (TypeError, ValueError):
        raise ValueError("pixel_size must be a number, got %r" % (pixel_size,))
    with np.errstate(over="ignore", under="ignore"):
        ok = bool(np.isfinite(np.float32(ps)) and ps > 0.0 and np.float32(ps) > 0.0)
    if not ok:
        raise ValueError("pixel_size must be finite and > 0, got %r" % (pixel_size,))
    c.pixel_size = ps
    c.interpolation = 1 if bilinear else 0
    return c


def shift_window(height, width, max_shift):
    """(H, W, S) of a translation registration, range-checked before any call into the library: H, W in 1..8192, S in 0..64,
    a template window (H - 2S) x (W - 2S) of 1..2^23 pixels"""
    h, w, s = _int_in(height, 1, 8192, "height"), _int_in(width, 1, 8192, "width"), _int_in(max_shift, 0, 64, "max_shift")
    if h <= 2 * s or w <= 2 * s:
        raise ValueError("a %d x %d image leaves no template window at max_shift %d" % (h, w, s))
    if (h - 2 * s) * (w - 2 * s) > 1 << 23:
        raise ValueError("the template window %d x %d holds more than 2^23 pixels" % (h - 2 * s, w - 2 * s))
    return h, w, s


def place_shape(n_rings, n_sectors):
    """(R, S) of a descriptor, range-checked before any call into the library: R in 1..64, S in 4..128, R * S <= 8192"""
    r, s = _int_in(n_rings, 1, 64, "n_rings"), _int_in(n_sectors, 4, 128, "n_sectors")
    if r * s > 8192:
        raise ValueError("n_rings * n_sectors must be at most 8192, got %d" % (r * s))
    return r, s


def place_config(n_rings, n_sectors, n_cells, n_angles, cell_begin=0, cell_end=None):
    """RRPlaceConfig for images [n_cells][n_angles], every field range-checked here; cell_end None: n_cells"""
    r, s = place_shape(n_rings, n_sectors)
    if cell_end is None:
        cell_end = n_cells
    for v in (cell_begin, cell_end):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("cell_begin and cell_end must be integers, got %r, %r" % (cell_begin, cell_end))
    if not 0 <= cell_begin < cell_end <= n_cells:
        raise ValueError("the cell window [%d, %d) must be non-empty and inside 0..%d" % (cell_begin, cell_end, n_cells))
    if r > cell_end - cell_begin:
        raise ValueError("%d rings in a window of %d cells" % (r, cell_end - cell_begin))
    if s > n_angles:
        raise ValueError("%d sectors in an image of %d columns" % (s, n_angles))
    c = RRPlaceConfig()
    c.cell_begin, c.cell_end, c.n_rings, c.n_sectors = int(cell_begin), int(cell_end), r, s
    return c


def _match_args(n_query, n_db, top_k):
    nq, n = _int_in(n_query, 1, 64, "n_query"), _int_in(n_db, 1, 1 << 28, "n_db")
    return nq, n, _int_in(top_k, 1, min(32, n), "top_k")


def _frames_arg(n_frames):
    return _int_in(n_frames, 1, 65535, "n_frames")


class _Scene:
    """What Context and MultiContext share: the error check and the nine scene setters.  _PREFIX selects the rr_ or the rr_multi_ entry
    points and with them the matching last-error function."""
    _PREFIX = "rr_"

    def _fn(self, name):
        return getattr(self._L, self._PREFIX + name)

    def _ck(self, rc):
        if rc != 0:
            raise RRError("%s (rc=%d)" % (self._fn("last_error")(self._h).decode(), rc))

    def set_mesh(self, verts, faces, face_object_id=None, builder="host"):
        v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
        f = np.ascontiguousarray(faces, np.uint32).reshape(-1, 3)
        o = None if face_object_id is None else np.ascontiguousarray(face_object_id, np.uint32)
        if o is not None and len(o) != len(f):
            raise ValueError("face_object_id must have one entry per face")
        fn = self._fn({"host": "set_mesh", "gpu": "set_mesh_gpu"}[builder])
        self._ck(fn(self._h, v.ctypes.data, len(v), f.ctypes.data, len(f), _ptr(o)))
        self.n_objects = int(o.max()) + 1 if o is not None and len(o) else 1

    # ---- dynamic scenes (include/radarays_mi355.h): the traced scene is every face's rest corners moved by its object's pose
    def set_object_poses(self, poses):
        """one rigid pose per object, [n_objects][7] = qx qy qz qw tx ty tz; the tree is refit in place (rr_set_object_poses)"""
        p = object_poses_array(poses)
        self._ck(self._fn("set_object_poses")(self._h, p.ctypes.data, len(p)))

    def update_vertices(self, verts):
        """new rest vertices (same count as the mesh's), poses kept (rr_update_vertices)"""
        v = vertex_array(verts)
        self._ck(self._fn("update_vertices")(self._h, v.ctypes.data, len(v)))

    def rebuild_tree(self, builder="host"):
        """a fresh tree of the posed scene ("host" SAH or "gpu" LBVH); rest geometry and poses stay (rr_rebuild_tree)"""
        b = builder_id(builder)
        self._ck(self._fn("rebuild_tree")(self._h, b))

    def set_materials(self, materials, object_materials, material_id_air=0):
        m = (RRMaterial * len(materials))(*[RRMaterial(*[float(x) for x in (t.astuple() if hasattr(t, "astuple") else t)])
                                            for t in materials])
        om = np.ascontiguousarray(object_materials, np.int32)
        self._ck(self._fn("set_materials")(self._h, m, len(materials), om.ctypes.data, len(om), int(material_id_air)))

    def set_config(self, cfg, n_angles=400, **kw):
        self.cfg = cfg
        self.n_angles = n_angles
        self._rrcfg = make_config(cfg, n_angles, **kw)
        self._ck(self._fn("set_config")(self._h, C.byref(self._rrcfg)))

    def set_beam_samples(self, dirs):
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        self._ck(self._fn("set_beam_samples")(self._h, d.ctypes.data, len(d)))

    def set_noise_offsets(self, rnd):
        """[n_angles] offsets, or [k][n_angles] (flat or 2-D): frame f of a batch uses row f % k."""
        r = np.ascontiguousarray(rnd, np.float32).ravel()
        self._ck(self._fn("set_noise_offsets")(self._h, r.ctypes.data, r.size))

    def set_motion_poses(self, poses):
        """include_motion: [n_angles][7] per-azimuth poses, or [k][n_angles][7] (frame f of a batch uses table f % k);
        None/empty switches it off."""
        if poses is None or len(poses) == 0:
            self._ck(self._fn("set_motion_poses")(self._h, None, 0))
            return
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 7)
        self._ck(self._fn("set_motion_poses")(self._h, p.ctypes.data, len(p)))


class Context(_Scene):
    """Owns one rr_ctx (one GPU)."""

    def __init__(self, device=0):
        self._L = lib()
        self._h = self._L.rr_create(int(device))
        if not self._h:
            raise RRError(self._L.rr_last_error(None).decode())
        self.device = int(device)
        self.cfg = None
        self.n_angles = 400
        self.n_objects = 1

    def close(self):
        if getattr(self, "_h", None):
            self._L.rr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def copy_mesh(self, src):
        """take the finished tree of another context (same or another device): rr_copy_mesh"""
        self._ck(self._L.rr_copy_mesh(self._h, src._h))
        self.n_objects = getattr(src, "n_objects", 1)

    def set_object_twists(self, twists=None):
        """one twist per object, [n_objects][6] = vx vy vz wx wy wz (map frame, about the map origin), read by the Doppler calls only;
        None or an empty array: every twist back to zero (rr_set_object_twists)"""
        t = np.zeros((0, 6), np.float32) if twists is None else np.ascontiguousarray(twists, np.float32)
        if t.size == 0:
            t = t.reshape(0, 6)
        if t.ndim != 2 or t.shape[1] != 6:
            raise ValueError("twists must be [n_objects][6] (vx vy vz wx wy wz), got %s" % (t.shape,))
        self._ck(self._L.rr_set_object_twists(self._h, t.ctypes.data if len(t) else None, len(t)))

    def tree_cost(self):
        """(cost of the current boxes, cost of the tree as built): rr_get_tree_cost; their ratio says when a rebuild pays"""
        a, b = C.c_double(), C.c_double()
        self._ck(self._L.rr_get_tree_cost(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def simulate(self, pose, az_begin=0, az_end=None, want_f32=False):
        """Host-buffer path (rr_simulate). Returns (u8 [n_cells][n_angles], f32|None, stats)."""
        p = np.ascontiguousarray(pose, np.float32)
        assert p.shape == (7,)
        if az_end is None:
            az_end = self.n_angles
        n_cells = self.cfg.n_cells if self.cfg is not None else 1   # unconfigured: the library reports it
        u8 = np.zeros((n_cells, self.n_angles), np.uint8)
        f32 = np.zeros((n_cells, self.n_angles), np.float32) if want_f32 else None
        st = RRStats()
        self._ck(self._L.rr_simulate(self._h, p.ctypes.data, az_begin, az_end, u8.ctypes.data, _ptr(f32), C.byref(st)))
        return u8, f32, st.asdict()

    def simulate_into(self, pose, out_u8):
        """rr_simulate into a preallocated uint8 [n_cells][n_angles] array, no statistics: the call a latency probe times."""
        p = np.ascontiguousarray(pose, np.float32)
        self._ck(self._L.rr_simulate(self._h, p.ctypes.data, 0, self.n_angles, out_u8.ctypes.data, None, None))

    def traversal_shape(self):
        """stats mode: wave-level loop shape of the last frame (rr_get_traversal_shape)."""
        a = np.zeros(8, np.uint64)
        self._ck(self._L.rr_get_traversal_shape(self._h, a.ctypes.data))
        return dict(zip(("waves", "iterations", "node_path_issues", "leaf_path_issues", "live_quad_steps", "max_iterations",
                         "node_steps", "leaf_steps"), (int(x) for x in a)))

    def simulate_columns_device(self, pose, az_begin, az_end, d_cols_u8_ptr, d_cols_f32_ptr=None, stream=None):
        p = np.ascontiguousarray(pose, np.float32)
        self._ck(self._L.rr_simulate_columns_device(self._h, p.ctypes.data, az_begin, az_end,
                                                    d_cols_u8_ptr, d_cols_f32_ptr, stream))

    def simulate_batch_device(self, poses, d_imgs_ptr, stream=None):
        """Whole frames of up to 64 (RR_MAX_BATCH) poses in one set of launches on `stream`: images [n][n_cells][n_angles] in HBM."""
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 7)
        self._ck(self._L.rr_simulate_batch_device(self._h, p.ctypes.data, len(p), d_imgs_ptr, stream))

    def simulate_batch_host_async(self, poses, h_imgs_ptr, stream=None):
        """Whole frames delivered to (page-locked) host memory [n][n_cells][n_angles]; complete after wait_host()."""
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 7)
        self._ck(self._L.rr_simulate_batch_host_async(self._h, p.ctypes.data, len(p), h_imgs_ptr, stream))

    def wait_host(self, h_imgs_ptr=None):
        self._ck(self._L.rr_wait_host(self._h, h_imgs_ptr))

    def copy_to_host_async(self, d_src_ptr, h_dst_ptr, nbytes, stream=None):
        """device -> host on `stream` by the library's own copy kernel (page-locked destination) -- rr_copy_to_host_async"""
        self._ck(lib().rr_copy_to_host_async(self._h, C.c_void_p(d_src_ptr), C.c_void_p(h_dst_ptr), C.c_size_t(nbytes), C.c_void_p(stream)))

    def host_delivery_route(self):
        """rr_host_delivery_route: "sdma" (ROCr's SDMA path in use), "sdma (untried)" or "stream copies" (a stream-ordered copy behind each batch)"""
        return {2: "sdma", 1: "sdma (untried)", 0: "stream copies"}.get(int(lib().rr_host_delivery_route(self._h)), "?")

    def deliver_to_host_async(self, d_src_ptr, h_dst_ptr, nbytes, stream=None):
        """device -> page-locked host over SDMA once `stream` has got here; complete after wait_host(h_dst_ptr) -- rr_deliver_to_host_async"""
        self._ck(lib().rr_deliver_to_host_async(self._h, C.c_void_p(d_src_ptr), C.c_void_p(h_dst_ptr), C.c_size_t(nbytes), C.c_void_p(stream)))

    def simulate_batch_columns_device(self, poses, az_begin, az_end, d_cols_u8_ptr, stream=None):
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 7)
        self._ck(self._L.rr_simulate_batch_columns_device(self._h, p.ctypes.data, len(p), az_begin, az_end,
                                                          d_cols_u8_ptr, stream))

    def assemble_image_device(self, d_cols_u8_ptr, d_img_ptr, stream=None):
        self._ck(self._L.rr_assemble_image_device(self._h, d_cols_u8_ptr, d_img_ptr, stream))

    def assemble_blocks_device(self, d_cols_u8_ptr, n_loc, block_stride, d_img_ptr, stream=None):
        self._ck(self._L.rr_assemble_blocks_device(self._h, d_cols_u8_ptr, int(n_loc), int(block_stride), d_img_ptr, stream))

    def assemble_frames_device(self, d_cols_u8_ptr, n_loc, block_stride, n_frames, frame_stride, d_imgs_ptr, stream=None):
        self._ck(self._L.rr_assemble_frames_device(self._h, d_cols_u8_ptr, int(n_loc), int(block_stride), int(n_frames),
                                                   int(frame_stride), d_imgs_ptr, stream))

    @staticmethod
    def _material_sets(sets):
        a = np.ascontiguousarray(np.asarray(sets, dtype=np.float32))
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError("material sets must have shape [n_sets][n_materials][4] (velocity, ambient, diffuse, specular)")
        return a

    def simulate_material_sets_device(self, pose, sets, d_imgs_ptr, stream=None):
        """n_sets material tables, one pose -> images [n_sets][n_cells][n_angles] in HBM."""
        a = self._material_sets(sets)
        p = np.ascontiguousarray(pose, dtype=np.float32)
        self._ck(self._L.rr_simulate_material_sets_device(self._h, p.ctypes.data, a.ctypes.data, a.shape[0], a.shape[1], d_imgs_ptr, stream))

    def simulate_material_sets(self, pose, sets):
        """Host-buffer variant: returns a uint8 array [n_sets][n_cells][n_angles]."""
        a = self._material_sets(sets)
        p = np.ascontiguousarray(pose, dtype=np.float32)
        n_cells = self.cfg.n_cells if self.cfg is not None else 1
        out = np.zeros((a.shape[0], n_cells, self.n_angles), dtype=np.uint8)
        self._ck(self._L.rr_simulate_material_sets(self._h, p.ctypes.data, a.ctypes.data, a.shape[0], a.shape[1], out.ctypes.data))
        return out

    @staticmethod
    def _param_sets(sets):
        """sets: iterable of dicts {"materials": [n_mat][4] or None, "beam_dirs": [n_beam][3] or None, "n_reflections": int or None}
        -> (ctypes array, the numpy arrays it points into, n_materials or None)"""
        keep, n_mat = [], None
        arr = (RRParamSet * len(sets))()
        for k, st in enumerate(sets):
            m = st.get("materials")
            if m is not None:
                m = np.ascontiguousarray(np.asarray([(t.astuple() if hasattr(t, "astuple") else t) for t in m], dtype=np.float32))
                if m.ndim != 2 or m.shape[1] != 4:
                    raise ValueError("materials of a set must have shape [n_materials][4]")
                n_mat = m.shape[0] if n_mat is None else n_mat
                keep.append(m)
                arr[k].materials = m.ctypes.data
            b = st.get("beam_dirs")
            if b is not None:
                b = np.ascontiguousarray(b, np.float32).reshape(-1, 3)
                keep.append(b)
                arr[k].beam_dirs = b.ctypes.data
            nr = st.get("n_reflections")
            arr[k].n_reflections = -1 if nr is None else int(nr)
        return arr, keep, n_mat

    def simulate_param_sets(self, pose, sets, n_materials, ref_u8=None, want_images=True, metrics=None, win_size=7):
        """rr_simulate_param_sets: one pose, n parameter sets (see _param_sets).  Returns (images uint8
        [n][n_cells][n_angles] or None, psnr float64 [n] or None against ref_u8).  With `metrics` (a METRIC_* mask or names,
        see metrics_mask) the second value is a METRICS_DTYPE array [n] instead: rr_simulate_param_sets_metrics."""
        arr, keep, n_mat = self._param_sets(sets)
        p = np.ascontiguousarray(pose, dtype=np.float32)
        n_cells = self.cfg.n_cells if self.cfg is not None else 1
        out = np.zeros((len(sets), n_cells, self.n_angles), dtype=np.uint8) if want_images else None
        if metrics is not None:
            which = metrics_mask(metrics)
            win = _win_arg(which, win_size)
            ref = None if ref_u8 is None else np.ascontiguousarray(ref_u8, np.uint8)
            if ref is None or ref.shape != (n_cells, self.n_angles):
                raise ValueError("metrics need a reference image [n_cells][n_angles] uint8")
            rec = np.zeros(len(sets), METRICS_DTYPE)
            self._ck(self._L.rr_simulate_param_sets_metrics(self._h, p.ctypes.data, arr, len(sets), int(n_materials),
                                                            _ptr(out), ref.ctypes.data, which, win, rec.ctypes.data))
            return out, rec
        psnr = ref = None
        if ref_u8 is not None:
            ref = np.ascontiguousarray(ref_u8, np.uint8)
            if ref.shape != (n_cells, self.n_angles):
                raise ValueError("reference image must be [n_cells][n_angles] uint8")
            psnr = np.zeros(len(sets), np.float64)
        self._ck(self._L.rr_simulate_param_sets(self._h, p.ctypes.data, arr, len(sets), int(n_materials), _ptr(out), _ptr(ref), _ptr(psnr)))
        return out, psnr

    def simulate_param_sets_device(self, pose, sets, n_materials, d_imgs_ptr, stream=None):
        arr, keep, _ = self._param_sets(sets)
        p = np.ascontiguousarray(pose, dtype=np.float32)
        self._ck(self._L.rr_simulate_param_sets_device(self._h, p.ctypes.data, arr, len(sets), int(n_materials), d_imgs_ptr, stream))

    def score_images_device(self, d_imgs_ptr, n_images, d_ref_ptr, stream=None, want_sse=False):
        """rr_score_images_device -> psnr float64 [n] (and the exact sums of squared differences uint64 [n])."""
        psnr = np.zeros(n_images, np.float64); sse = np.zeros(n_images, np.uint64)
        self._ck(self._L.rr_score_images_device(self._h, d_imgs_ptr, int(n_images), d_ref_ptr, psnr.ctypes.data, sse.ctypes.data, stream))
        return (psnr, sse) if want_sse else psnr

    # ---- images against one reference image (rr_metrics.hip): PSNR, SSIM, joint histogram and its entropies
    def compare_images_device(self, d_imgs_ptr, n_images, d_ref_ptr, which=METRIC_ALL, win_size=7, d_joint_hist_ptr=None, stream=None):
        """rr_compare_images_device: n images [n][n_cells][n_angles] and one reference image in HBM -> METRICS_DTYPE array [n];
        d_joint_hist_ptr (HBM, uint32 [n][256][256]) receives the joint histograms.  Synchronous on `stream`."""
        self._polar_shape()
        which = metrics_mask(which)
        win = _win_arg(which, win_size)
        n = _frames_arg(n_images)
        if not d_imgs_ptr or not d_ref_ptr:
            raise ValueError("compare_images_device needs image and reference buffers")
        rec = np.zeros(n, METRICS_DTYPE)
        self._ck(self._L.rr_compare_images_device(self._h, d_imgs_ptr, n, d_ref_ptr, which, win, rec.ctypes.data, d_joint_hist_ptr, stream))
        return rec

    def compare_images(self, imgs, ref, which=METRIC_ALL, win_size=7, want_hist=False):
        """rr_compare_images on host images [n][n_cells][n_angles] (or one image) against ref [n_cells][n_angles] ->
        METRICS_DTYPE array [n], and with want_hist the joint histograms uint32 [n][256][256] as well"""
        x = self._polar_images(imgs)
        r = self._one_reference(ref)
        which = metrics_mask(which)
        win = _win_arg(which, win_size)
        rec = np.zeros(len(x), METRICS_DTYPE)
        hist = np.zeros((len(x), 256, 256), np.uint32) if want_hist else None
        self._ck(self._L.rr_compare_images(self._h, x.ctypes.data, len(x), r.ctypes.data, which, win, rec.ctypes.data, _ptr(hist)))
        return (rec, hist) if want_hist else rec

    # ---- azimuth registration (rr_align.hip): the circular cross-correlation of images with one reference over all shifts
    def _cell_window(self, cell_begin, cell_end):
        """(cell_begin, cell_end) of a window inside this context's image, at most 2^23 pixels; cell_end None: n_cells"""
        n_cells, n_angles = self._polar_shape()
        if cell_end is None:
            cell_end = n_cells
        for v in (cell_begin, cell_end):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError("cell_begin and cell_end must be integers, got %r, %r" % (cell_begin, cell_end))
        if not 0 <= cell_begin < cell_end <= n_cells:
            raise ValueError("the cell window [%d, %d) must be non-empty and inside 0..%d" % (cell_begin, cell_end, n_cells))
        if (cell_end - cell_begin) * n_angles > 1 << 23:
            raise ValueError("the cell window [%d, %d) x %d azimuths holds more than 2^23 pixels" % (cell_begin, cell_end, n_angles))
        return int(cell_begin), int(cell_end)

    def align_images_device(self, d_imgs_ptr, n_images, d_ref_ptr, cell_begin=0, cell_end=None, d_xcorr_ptr=None, stream=None):
        """rr_align_images_device: n images [n][n_cells][n_angles] and one reference image in HBM -> ALIGN_DTYPE array [n] (the
        best circular azimuth shift and the scores at it); d_xcorr_ptr (HBM, int64 [n][n_angles]) receives xcorr at every shift.
        Synchronous on `stream`."""
        cb, ce = self._cell_window(cell_begin, cell_end)
        n = _frames_arg(n_images)
        if not d_imgs_ptr or not d_ref_ptr:
            raise ValueError("align_images_device needs image and reference buffers")
        rec = np.zeros(n, ALIGN_DTYPE)
        self._ck(self._L.rr_align_images_device(self._h, d_imgs_ptr, n, d_ref_ptr, cb, ce, rec.ctypes.data, d_xcorr_ptr, stream))
        return rec

    def align_images(self, imgs, ref, cell_begin=0, cell_end=None, want_curve=False):
        """rr_align_images on host images [n][n_cells][n_angles] (or one image) against ref [n_cells][n_angles] -> ALIGN_DTYPE
        array [n], and with want_curve xcorr int64 [n][n_angles] as well"""
        x = self._polar_images(imgs)
        r = self._one_reference(ref)
        cb, ce = self._cell_window(cell_begin, cell_end)
        rec = np.zeros(len(x), ALIGN_DTYPE)
        curve = np.zeros((len(x), self.n_angles), np.int64) if want_curve else None
        self._ck(self._L.rr_align_images(self._h, x.ctypes.data, len(x), r.ctypes.data, cb, ce, rec.ctypes.data, _ptr(curve)))
        return (rec, curve) if want_curve else rec

    def simulate_batch_align(self, poses, ref, cell_begin=0, cell_end=None, want_images=False, want_curve=False):
        """rr_simulate_batch_align: up to 64 poses simulated and registered against ref [n_cells][n_angles] ->
        (images uint8 [n][n_cells][n_angles] or None, ALIGN_DTYPE array [n], xcorr int64 [n][n_angles] or None)"""
        r = self._one_reference(ref)
        cb, ce = self._cell_window(cell_begin, cell_end)
        p = _pose_batch(poses)
        n_cells, n_angles = self._polar_shape()
        out = np.zeros((len(p), n_cells, n_angles), np.uint8) if want_images else None
        rec = np.zeros(len(p), ALIGN_DTYPE)
        curve = np.zeros((len(p), n_angles), np.int64) if want_curve else None
        self._ck(self._L.rr_simulate_batch_align(self._h, p.ctypes.data, len(p), r.ctypes.data, cb, ce, _ptr(out), rec.ctypes.data, _ptr(curve)))
        return out, rec, curve

    # ---- translation registration (rr_shift.hip): the 2-D cross-correlation of images [H][W] with one reference over -S..S pixels
    def shift_images_device(self, d_imgs_ptr, n_images, d_ref_ptr, height, width, max_shift, d_xcorr_ptr=None, d_sse_ptr=None, stream=None):
        """rr_shift_images_device: n images [n][H][W] and one reference image in HBM -> SHIFT_DTYPE array [n] (the best shift and
        the scores at it); d_xcorr_ptr (int64) and d_sse_ptr (uint64), HBM [n][2S+1][2S+1], receive the surfaces.  Synchronous
        on `stream`.  Needs no config."""
        h, w, s = shift_window(height, width, max_shift)
        n = _frames_arg(n_images)
        if not d_imgs_ptr or not d_ref_ptr:
            raise ValueError("shift_images_device needs image and reference buffers")
        rec = np.zeros(n, SHIFT_DTYPE)
        self._ck(self._L.rr_shift_images_device(self._h, d_imgs_ptr, n, d_ref_ptr, h, w, s, rec.ctypes.data, d_xcorr_ptr, d_sse_ptr, stream))
        return rec

    def shift_images(self, imgs, ref, max_shift, want_surfaces=False):
        """rr_shift_images on host images uint8 [n][H][W] (or one image) against ref [H][W] -> SHIFT_DTYPE array [n], and with
        want_surfaces (records, xcorr int64 [n][2S+1][2S+1], sse uint64 [n][2S+1][2S+1])"""
        x, r = np.asarray(imgs), np.asarray(ref)
        if x.dtype != np.uint8 or r.dtype != np.uint8:
            raise ValueError("images must be uint8, got %s and %s" % (x.dtype, r.dtype))
        if x.ndim == 2:
            x = x[None]
        if x.ndim != 3 or r.ndim != 2 or x.shape[1:] != r.shape or not 1 <= x.shape[0] <= 65535:
            raise ValueError("images [n][H][W] (n in 1..65535) and one reference [H][W] of the same shape, got %s and %s" % (np.asarray(imgs).shape, r.shape))
        h, w, s = shift_window(r.shape[0], r.shape[1], max_shift)
        x, r = np.ascontiguousarray(x), np.ascontiguousarray(r)
        d = 2 * s + 1
        rec = np.zeros(len(x), SHIFT_DTYPE)
        xc = np.zeros((len(x), d, d), np.int64) if want_surfaces else None
        sse = np.zeros((len(x), d, d), np.uint64) if want_surfaces else None
        self._ck(self._L.rr_shift_images(self._h, x.ctypes.data, len(x), r.ctypes.data, h, w, s, rec.ctypes.data, _ptr(xc), _ptr(sse)))
        return (rec, xc, sse) if want_surfaces else rec

    def simulate_batch_shift(self, poses, ref_polar, width, pixel_size, max_shift, bilinear=True, want_images=False, want_xcorr=False):
        """rr_simulate_batch_shift: up to 64 poses simulated, their images and ref_polar [n_cells][n_angles] made Cartesian
        (width x width, pixel_size m/pixel) and registered over -S..S pixels -> (Cartesian images uint8 [n][width][width] or
        None, SHIFT_DTYPE array [n], xcorr int64 [n][2S+1][2S+1] or None)"""
        r = self._one_reference(ref_polar)
        c = cartesian_config(width, pixel_size, bilinear)
        _, _, s = shift_window(c.width, c.width, max_shift)
        p = _pose_batch(poses)
        d = 2 * s + 1
        out = np.zeros((len(p), c.width, c.width), np.uint8) if want_images else None
        rec = np.zeros(len(p), SHIFT_DTYPE)
        xc = np.zeros((len(p), d, d), np.int64) if want_xcorr else None
        self._ck(self._L.rr_simulate_batch_shift(self._h, p.ctypes.data, len(p), r.ctypes.data, C.byref(c), s, _ptr(out), rec.ctypes.data,
                                                 _ptr(xc)))
        return out, rec, xc

    # ---- place recognition (rr_place.hip): ring/sector descriptors of polar images and their exact matching
    def _place_cfg(self, place_cfg):
        """an RRPlaceConfig, a dict or a tuple (n_rings, n_sectors[, cell_begin[, cell_end]]) -> a checked RRPlaceConfig for this context's images"""
        n_cells, n_angles = self._polar_shape()
        if isinstance(place_cfg, RRPlaceConfig):
            return place_config(place_cfg.n_rings, place_cfg.n_sectors, n_cells, n_angles, place_cfg.cell_begin, place_cfg.cell_end)
        if isinstance(place_cfg, dict):
            return place_config(n_cells=n_cells, n_angles=n_angles, **place_cfg)
        return place_config(place_cfg[0], place_cfg[1], n_cells, n_angles, *place_cfg[2:])

    def describe_images_device(self, d_imgs_ptr, n_images, place_cfg, d_desc_ptr, stream=None):
        """rr_describe_images_device: n images [n][n_cells][n_angles] in HBM -> descriptors uint8 [n][R][S] in HBM, enqueued on `stream`"""
        p = self._place_cfg(place_cfg)
        n = _frames_arg(n_images)
        if not d_imgs_ptr or not d_desc_ptr:
            raise ValueError("describe_images_device needs image and descriptor buffers")
        self._ck(self._L.rr_describe_images_device(self._h, d_imgs_ptr, n, C.byref(p), d_desc_ptr, stream))

    def describe_images(self, imgs, place_cfg):
        """rr_describe_images on host images [n][n_cells][n_angles] (or one image) -> descriptors uint8 [n][R][S]"""
        x = self._polar_images(imgs)
        p = self._place_cfg(place_cfg)
        out = np.zeros((len(x), p.n_rings, p.n_sectors), np.uint8)
        self._ck(self._L.rr_describe_images(self._h, x.ctypes.data, len(x), C.byref(p), out.ctypes.data))
        return out

    def simulate_batch_describe(self, poses, place_cfg):
        """rr_simulate_batch_describe: up to 64 poses simulated and described, no image leaving the GPU -> uint8 [n][R][S]"""
        p = self._place_cfg(place_cfg)
        ps = _pose_batch(poses)
        out = np.zeros((len(ps), p.n_rings, p.n_sectors), np.uint8)
        self._ck(self._L.rr_simulate_batch_describe(self._h, ps.ctypes.data, len(ps), C.byref(p), out.ctypes.data))
        return out

    def match_descriptors_device(self, d_query_ptr, n_query, d_db_ptr, n_db, n_rings, n_sectors, top_k, d_sse_ptr=None, d_shift_ptr=None, stream=None):
        """rr_match_descriptors_device: queries [n_query][R][S] against a database [n_db][R][S], both in HBM -> PLACE_DTYPE array
        [n_query][top_k], ranked by (sse, index); d_sse_ptr (uint32) and d_shift_ptr (uint16, only with d_sse_ptr), HBM [n_query][n_db],
        receive every pair's SSE and shift.  Synchronous on `stream`.  Needs no config."""
        r, s = place_shape(n_rings, n_sectors)
        nq, n, k = _match_args(n_query, n_db, top_k)
        if not d_query_ptr or not d_db_ptr:
            raise ValueError("match_descriptors_device needs query and database buffers")
        if d_shift_ptr and not d_sse_ptr:
            raise ValueError("d_shift_ptr comes with d_sse_ptr")
        rec = np.zeros((nq, k), PLACE_DTYPE)
        self._ck(self._L.rr_match_descriptors_device(self._h, d_query_ptr, nq, d_db_ptr, n, r, s, k, rec.ctypes.data, d_sse_ptr, d_shift_ptr, stream))
        return rec

    def match_descriptors(self, query, db, top_k, want_full=False):
        """rr_match_descriptors on host descriptors: query uint8 [n_query][R][S] (or one [R][S]) against db [n_db][R][S] ->
        PLACE_DTYPE array [n_query][top_k], and with want_full (records, sse uint32 [n_query][n_db], shift uint16 [n_query][n_db])"""
        q, d = np.asarray(query), np.asarray(db)
        if q.dtype != np.uint8 or d.dtype != np.uint8:
            raise ValueError("descriptors must be uint8, got %s and %s" % (q.dtype, d.dtype))
        if q.ndim == 2:
            q = q[None]
        if q.ndim != 3 or d.ndim != 3 or q.shape[1:] != d.shape[1:]:
            raise ValueError("queries [n_query][R][S] and a database [n_db][R][S] of the same R, S, got %s and %s" % (np.asarray(query).shape, d.shape))
        r, s = place_shape(q.shape[1], q.shape[2])
        nq, n, k = _match_args(q.shape[0], d.shape[0], top_k)
        q, d = np.ascontiguousarray(q), np.ascontiguousarray(d)
        rec = np.zeros((nq, k), PLACE_DTYPE)
        sse = np.zeros((nq, n), np.uint32) if want_full else None
        shift = np.zeros((nq, n), np.uint16) if want_full else None
        self._ck(self._L.rr_match_descriptors(self._h, q.ctypes.data, nq, d.ctypes.data, n, r, s, k, rec.ctypes.data, _ptr(sse), _ptr(shift)))
        return (rec, sse, shift) if want_full else rec

    def simulate_device(self, pose, d_img_ptr, stream=None):
        p = np.ascontiguousarray(pose, np.float32)
        self._ck(self._L.rr_simulate_device(self._h, p.ctypes.data, d_img_ptr, stream))

    # ---- point clouds and Cartesian images from polar images (rr_detect.hip): any context with a config, mesh or not
    def _polar_shape(self):
        if self.cfg is None:
            raise RRError("rr_set_config has not been called")
        return int(self.cfg.n_cells), int(self.n_angles)

    def _one_reference(self, ref):
        """the one reference image [n_cells][n_angles] of a comparison, as _polar_images returns it"""
        r = self._polar_images(ref)
        if len(r) != 1:
            raise ValueError("one reference image, got %d" % len(r))
        return r

    def _polar_images(self, imgs):
        """uint8 [n][n_cells][n_angles] (or one [n_cells][n_angles] image) of this context's shape -> contiguous 3-D array"""
        n_cells, n_angles = self._polar_shape()
        x = np.asarray(imgs)
        if x.dtype != np.uint8:
            raise ValueError("polar images must be uint8, got dtype %s" % x.dtype)
        if x.ndim == 2:
            x = x[None]
        if x.ndim != 3 or x.shape[1:] != (n_cells, n_angles) or not 1 <= x.shape[0] <= 65535:
            raise ValueError("polar images must have shape [n][%d][%d] (n in 1..65535), got %s" % (n_cells, n_angles, np.asarray(imgs).shape))
        return np.ascontiguousarray(x)

    def detect_device(self, d_imgs_ptr, n_frames, cfg=None, d_points_ptr=None, max_points=0, d_offsets_ptr=None, stream=None, **kw):
        """rr_detect_device: points [n_frames][max_points] (rr_radar_point, POINT_DTYPE) and offsets [n_frames][n_angles + 1]
        (uint32) in HBM, on `stream`.  max_points = 0 counts only."""
        n_cells, _ = self._polar_shape()
        c = detect_config(cfg, n_cells=n_cells, **kw)
        n = _frames_arg(n_frames)
        mp = _int_in(max_points, 0, 2**31 - 1, "max_points")
        if not d_imgs_ptr or not d_offsets_ptr or (mp > 0 and not d_points_ptr):
            raise ValueError("detect_device needs image and offset buffers (and a point buffer when max_points > 0)")
        self._ck(self._L.rr_detect_device(self._h, d_imgs_ptr, n, C.byref(c), d_points_ptr, mp, d_offsets_ptr, stream))

    def detect(self, imgs, cfg=None, max_points=None, allow_truncation=False, **kw):
        """rr_detect on host images [n][n_cells][n_angles] (or one image).  Returns (list of n POINT_DTYPE arrays, offsets
        uint32 [n][n_angles + 1]); offsets[f][c] = points of frame f in columns before c, offsets[f][-1] = the true total.
        max_points None: room for every detection (a count-only call first).  A frame with more detections than max_points
        raises RRError naming it, unless allow_truncation=True (then it holds its first max_points points)."""
        x = self._polar_images(imgs)
        n_cells, n_angles = self._polar_shape()
        c = detect_config(cfg, n_cells=n_cells, **kw)
        n = len(x)
        offs = np.zeros((n, n_angles + 1), np.uint32)
        if max_points is None:
            self._ck(self._L.rr_detect(self._h, x.ctypes.data, n, C.byref(c), None, 0, offs.ctypes.data))
            max_points = int(offs[:, -1].max())
        mp = _int_in(max_points, 0, 2**31 - 1, "max_points")
        pts = np.zeros((n, max(mp, 1)), POINT_DTYPE)
        self._ck(self._L.rr_detect(self._h, x.ctypes.data, n, C.byref(c), pts.ctypes.data if mp else None, mp, offs.ctypes.data))
        totals = offs[:, -1]
        over = np.nonzero(totals > mp)[0]
        if len(over) and not allow_truncation:
            f = int(over[0])
            raise RRError("detect: frame %d has %d detections, max_points is %d (%d frame(s) truncated)" % (f, int(totals[f]), mp, len(over)))
        return [pts[f, :min(int(totals[f]), mp)].copy() for f in range(n)], offs

    # ---- windowed CFAR (rr_window.hip): the same outputs as detect, and the detection mask
    def detect_window_device(self, d_imgs_ptr, n_frames, cfg=None, d_points_ptr=None, max_points=0, d_offsets_ptr=None, d_mask_ptr=None, stream=None, **kw):
        """rr_detect_window_device: points and offsets as detect_device, and with d_mask_ptr the uint8 mask [n_frames][n_cells][n_angles]
        (255 at a detection), all in HBM, on `stream`.  max_points = 0 counts only."""
        n_cells, n_angles = self._polar_shape()
        c = window_detect_config(cfg, n_cells=n_cells, n_angles=n_angles, **kw)
        n = _frames_arg(n_frames)
        mp = _int_in(max_points, 0, 2**31 - 1, "max_points")
        if not d_imgs_ptr or not d_offsets_ptr or (mp > 0 and not d_points_ptr):
            raise ValueError("detect_window_device needs image and offset buffers (and a point buffer when max_points > 0)")
        self._ck(self._L.rr_detect_window_device(self._h, d_imgs_ptr, n, C.byref(c), d_points_ptr, mp, d_offsets_ptr, d_mask_ptr, stream))

    def detect_window(self, imgs, cfg=None, max_points=None, mask=False, allow_truncation=False, **kw):
        """rr_detect_window on host images [n][n_cells][n_angles] (or one image).  Returns (list of n POINT_DTYPE arrays, offsets uint32
        [n][n_angles + 1]) as detect does, and with mask=True a third value, the uint8 mask [n][n_cells][n_angles].  max_points None:
        room for every detection (a count-only call first); a truncated frame raises RRError unless allow_truncation=True."""
        x = self._polar_images(imgs)
        n_cells, n_angles = self._polar_shape()
        c = window_detect_config(cfg, n_cells=n_cells, n_angles=n_angles, **kw)
        n = len(x)
        offs = np.zeros((n, n_angles + 1), np.uint32)
        if max_points is None:
            self._ck(self._L.rr_detect_window(self._h, x.ctypes.data, n, C.byref(c), None, 0, offs.ctypes.data, None))
            max_points = int(offs[:, -1].max())
        mp = _int_in(max_points, 0, 2**31 - 1, "max_points")
        pts = np.zeros((n, max(mp, 1)), POINT_DTYPE)
        m = np.zeros(x.shape, np.uint8) if mask else None
        self._ck(self._L.rr_detect_window(self._h, x.ctypes.data, n, C.byref(c), pts.ctypes.data if mp else None, mp, offs.ctypes.data, _ptr(m)))
        totals = offs[:, -1]
        over = np.nonzero(totals > mp)[0]
        if len(over) and not allow_truncation:
            f = int(over[0])
            raise RRError("detect_window: frame %d has %d detections, max_points is %d (%d frame(s) truncated)" % (f, int(totals[f]), mp, len(over)))
        clouds = [pts[f, :min(int(totals[f]), mp)].copy() for f in range(n)]
        return (clouds, offs, m) if mask else (clouds, offs)

    def polar_to_cartesian_device(self, d_imgs_ptr, n_frames, width, pixel_size, d_out_ptr, bilinear=True, stream=None):
        """rr_polar_to_cartesian_device: [n_frames][width][width] uint8 in HBM, on `stream`"""
        self._polar_shape()
        c = cartesian_config(width, pixel_size, bilinear)
        n = _frames_arg(n_frames)
        if not d_imgs_ptr or not d_out_ptr:
            raise ValueError("polar_to_cartesian_device needs image and output buffers")
        self._ck(self._L.rr_polar_to_cartesian_device(self._h, d_imgs_ptr, n, C.byref(c), d_out_ptr, stream))

    def polar_to_cartesian(self, imgs, width, pixel_size, bilinear=True):
        """rr_polar_to_cartesian on host images [n][n_cells][n_angles] (or one image) -> uint8 [n][width][width]"""
        x = self._polar_images(imgs)
        c = cartesian_config(width, pixel_size, bilinear)
        out = np.zeros((len(x), c.width, c.width), np.uint8)
        self._ck(self._L.rr_polar_to_cartesian(self._h, x.ctypes.data, len(x), C.byref(c), out.ctypes.data))
        return out

    # ---- sweep compensation (rr_deskew.hip): motion and Doppler distortion taken out again; any context with a config, mesh or not
    def _sweep_inputs(self, az_poses, ref_poses, sensor_vel, gain):
        """(az [n][n_angles][7], ref [n][7], vel [n][3] or None, gain), shape- and value-checked before any call into the library"""
        _, n_angles = self._polar_shape()
        ref = _rows(ref_poses, 7, "reference poses")
        az = np.asarray(az_poses)
        if az.dtype.kind not in "fiu":
            raise ValueError("azimuth poses must be real numbers, got dtype %s" % az.dtype)
        if az.ndim == 2:
            az = az[None]
        if az.ndim != 3 or az.shape != (len(ref), n_angles, 7) or not 1 <= len(ref) <= 65535:
            raise ValueError("azimuth poses must have shape [n][%d][7] with one reference pose [7] per frame (n in 1..65535), got %s and %s"
                             % (n_angles, np.asarray(az_poses).shape, np.asarray(ref_poses).shape))
        az = np.ascontiguousarray(az, np.float32)
        vel = None if sensor_vel is None else _rows(sensor_vel, 3, "sensor velocities")
        if vel is not None and len(vel) != len(ref):
            raise ValueError("sensor_vel must hold one velocity per frame: %d frames, %d velocities" % (len(ref), len(vel)))
        try:
            g = float(gain)
        except (TypeError, ValueError):
            raise ValueError("gain must be a number, got %r" % (gain,))
        with np.errstate(over="ignore"):
            if not np.isfinite(np.float32(g)):
                raise ValueError("gain must be finite, got %r" % (gain,))
        return az, ref, vel, g

    def _sweep_records(self, table, n_frames):
        """SWEEP_DTYPE [n_frames][n_angles] (or one frame's [n_angles]) of this context's shape -> contiguous 2-D array"""
        _, n_angles = self._polar_shape()
        t = np.asarray(table)
        if t.dtype != SWEEP_DTYPE:
            raise ValueError("a sweep table must have dtype SWEEP_DTYPE, got %s" % t.dtype)
        if t.ndim == 1:
            t = t[None]
        if t.shape != (n_frames, n_angles):
            raise ValueError("the sweep table must have shape [%d][%d], got %s" % (n_frames, n_angles, np.asarray(table).shape))
        return np.ascontiguousarray(t)

    def sweep_table_device(self, d_az_poses_ptr, d_ref_poses_ptr, n_frames, d_table_ptr, d_sensor_vel_ptr=None, gain=0.0, stream=None):
        """rr_sweep_table_device: SWEEP_DTYPE records [n_frames][n_angles] in HBM (16-byte aligned) from float32 poses [n_frames][n_angles][7],
        reference poses [n_frames][7] and optionally velocities [n_frames][3] in HBM, on `stream`"""
        self._polar_shape()
        n = _frames_arg(n_frames)
        if not d_az_poses_ptr or not d_ref_poses_ptr or not d_table_ptr:
            raise ValueError("sweep_table_device needs pose, reference pose and table buffers")
        g = float(gain)
        if not np.isfinite(g):
            raise ValueError("gain must be finite, got %r" % (gain,))
        self._ck(self._L.rr_sweep_table_device(self._h, d_az_poses_ptr, d_ref_poses_ptr, d_sensor_vel_ptr, g, n, d_table_ptr, stream))

    def sweep_table(self, az_poses, ref_poses, sensor_vel=None, gain=0.0):
        """rr_sweep_table: per-azimuth poses [n][n_angles][7] (the table set_motion_poses takes; or one frame's [n_angles][7]), reference
        poses [n][7] and optionally map-frame sensor velocities [n][3] with the Doppler `gain` -> SWEEP_DTYPE [n][n_angles]"""
        az, ref, vel, g = self._sweep_inputs(az_poses, ref_poses, sensor_vel, gain)
        table = np.zeros(az.shape[:2], SWEEP_DTYPE)
        self._ck(self._L.rr_sweep_table(self._h, az.ctypes.data, ref.ctypes.data, _ptr(vel), g, len(ref),
                                        table.ctypes.data))
        return table

    def compensate_points_device(self, d_points_ptr, d_offsets_ptr, n_frames, max_points, d_table_ptr, d_out_ptr=None, stream=None):
        """rr_compensate_points_device: the points rr_detect_device wrote, moved into the reference frame; d_out_ptr None: in place"""
        self._polar_shape()
        n, mp = _frames_arg(n_frames), _int_in(max_points, 0, 2**31 - 1, "max_points")
        if not d_offsets_ptr or not d_table_ptr or (mp > 0 and not d_points_ptr):
            raise ValueError("compensate_points_device needs point, offset and table buffers")
        self._ck(self._L.rr_compensate_points_device(self._h, d_points_ptr, d_offsets_ptr, n, mp, d_table_ptr, d_out_ptr or d_points_ptr, stream))

    def compensate_points(self, points, offsets, table):
        """rr_compensate_points on what detect() returned: a list of n POINT_DTYPE arrays and offsets uint32 [n][n_angles + 1], with a
        sweep table SWEEP_DTYPE [n][n_angles] -> a list of n POINT_DTYPE arrays in the reference frame, same order and lengths"""
        _, n_angles = self._polar_shape()
        pts = _cloud_list(points)
        offs = _cloud_offsets(offsets, len(pts), n_angles)
        t = self._sweep_records(table, len(pts))      # a bad table is reported before a frame that does not hold its points
        buf, offs, lens = _clouds(pts, offs, n_angles, False)
        self._ck(self._L.rr_compensate_points(self._h, buf.ctypes.data, offs.ctypes.data, len(buf), buf.shape[1], t.ctypes.data, buf.ctypes.data))
        return [buf[f, :k].copy() for f, k in enumerate(lens)]

    @staticmethod
    def _iterations(iterations):
        return _int_in(iterations, 1, 8, "iterations")

    def polar_to_cartesian_sweep_device(self, d_imgs_ptr, n_frames, width, pixel_size, d_table_ptr, d_out_ptr, bilinear=True, iterations=2, stream=None):
        """rr_polar_to_cartesian_sweep_device: [n_frames][width][width] uint8 in the reference frame, in HBM, on `stream`"""
        _, n_angles = self._polar_shape()
        c = cartesian_config(width, pixel_size, bilinear)
        n, it = _frames_arg(n_frames), self._iterations(iterations)
        if n_angles * SWEEP_DTYPE.itemsize > 65536:
            raise ValueError("n_angles * 32 exceeds 65536: a frame's records do not fit in LDS")
        if not d_imgs_ptr or not d_table_ptr or not d_out_ptr:
            raise ValueError("polar_to_cartesian_sweep_device needs image, table and output buffers")
        self._ck(self._L.rr_polar_to_cartesian_sweep_device(self._h, d_imgs_ptr, n, C.byref(c), d_table_ptr, it, d_out_ptr, stream))

    def polar_to_cartesian_sweep(self, imgs, table, width, pixel_size, bilinear=True, iterations=2):
        """rr_polar_to_cartesian_sweep on host images [n][n_cells][n_angles] (or one image) and a sweep table SWEEP_DTYPE [n][n_angles]
        -> uint8 [n][width][width] in the reference frame"""
        x = self._polar_images(imgs)
        c = cartesian_config(width, pixel_size, bilinear)
        it = self._iterations(iterations)
        t = self._sweep_records(table, len(x))
        if x.shape[2] * SWEEP_DTYPE.itemsize > 65536:
            raise ValueError("n_angles * 32 exceeds 65536: a frame's records do not fit in LDS")
        out = np.zeros((len(x), c.width, c.width), np.uint8)
        self._ck(self._L.rr_polar_to_cartesian_sweep(self._h, x.ctypes.data, len(x), C.byref(c), t.ctypes.data, it, out.ctypes.data))
        return out

    # ---- scan matching (rr_icp.hip): planar point-to-point ICP of n clouds against one; any context with a config, mesh or not
    def register_points_device(self, d_points_ptr, d_offsets_ptr, n_frames, max_points, d_tgt_points_ptr, d_tgt_count_ptr, max_tgt, d_recs_ptr,
                               d_init_ptr=None, gate=1.0, iterations=10, d_corr_ptr=None, stream=None):
        """rr_register_points_device: ICP_DTYPE records [n_frames] in HBM from the points [n_frames][max_points] and offsets
        [n_frames][n_angles + 1] rr_detect_device wrote, against the target points [max_tgt] whose count is the uint32 at d_tgt_count_ptr;
        d_init_ptr: float64 [n_frames][4] or None (identity); d_corr_ptr: uint32 [n_frames][max_points] or None; on `stream`"""
        self._register_device("register_points_device", 1, d_points_ptr, d_offsets_ptr, n_frames, max_points,
                              d_tgt_points_ptr, d_tgt_count_ptr, max_tgt, d_recs_ptr, d_init_ptr, gate, iterations, d_corr_ptr, stream)

    def _register_device(self, name, tgt_align, d_points_ptr, d_offsets_ptr, n_frames, max_points, d_tgt_ptr, d_tgt_count_ptr, max_tgt, d_recs_ptr,
                         d_init_ptr, gate, iterations, d_corr_ptr, stream):
        """the device form of either matcher: rr_`name` of the library (looked up once every argument has passed), the target at a multiple of
        tgt_align bytes"""
        self._polar_shape()
        n = _frames_arg(n_frames)
        mp, mt = _int_in(max_points, 0, ICP_MAX_POINTS, "max_points"), _int_in(max_tgt, 0, ICP_MAX_POINTS, "max_tgt")
        it, g = _int_in(iterations, 0, 64, "iterations"), _icp_gate(gate)
        if not d_offsets_ptr or not d_tgt_count_ptr or not d_recs_ptr or (mp > 0 and not d_points_ptr) or (mt > 0 and not d_tgt_ptr):
            raise ValueError("%s needs point, offset, target, target count and record buffers" % name)
        if (d_tgt_ptr or 0) % tgt_align:
            raise ValueError("the target must be %d-byte aligned" % tgt_align)
        self._ck(getattr(self._L, "rr_" + name)(self._h, d_points_ptr, d_offsets_ptr, n, mp, d_tgt_ptr, d_tgt_count_ptr, mt, d_init_ptr, g, it, d_recs_ptr, d_corr_ptr, stream))

    def _register(self, name, pts, offsets, n_angles, tgt, init, gate, iterations, want_corr):
        """the host form of either matcher, rr_`name` of the library, on a validated cloud list and target array"""
        buf, offs, lens = _clouds(pts, offsets, n_angles, True)
        n, mp = buf.shape
        x0 = _icp_init(init, n)
        it, g = _int_in(iterations, 0, 64, "iterations"), _icp_gate(gate)
        recs = np.zeros(n, ICP_DTYPE)
        corr = np.full((n, mp), ICP_NONE, np.uint32) if want_corr else None
        self._ck(getattr(self._L, "rr_" + name)(self._h, buf.ctypes.data, offs.ctypes.data, n, mp, tgt.ctypes.data if len(tgt) else None, len(tgt), len(tgt),
                                                _ptr(x0), g, it, recs.ctypes.data, _ptr(corr)))
        if want_corr:
            return recs, [corr[f, :k].copy() for f, k in enumerate(lens)]
        return recs

    def register_points(self, points_list, offsets, target_points, init=None, gate=1.0, iterations=10, want_corr=False):
        """rr_register_points on what detect() (or compensate_points()) returned: a list of n POINT_DTYPE arrays and offsets uint32
        [n][n_angles + 1], against ONE target POINT_DTYPE array.  init: float64 [n][4] = (c, s, tx, ty) per cloud (se2_states makes it) or
        None for the identity; gate in metres; iterations 0..64 (0 scores the initial states).  Returns ICP_DTYPE [n]: the transform that
        maps each cloud into the target's frame, sse, n_matched and flags; with want_corr also a list of n uint32 arrays: the target index
        each point was matched to in the last pass, ICP_NONE for an unmatched point."""
        _, n_angles = self._polar_shape()
        pts = _cloud_list(points_list)
        tgt = _scan(target_points, None, "the target")      # a bad target is reported before a cloud over the cap, and is held to it too
        if len(tgt) > ICP_MAX_POINTS:
            raise ValueError("a cloud may hold at most %d points" % ICP_MAX_POINTS)
        return self._register("register_points", pts, offsets, n_angles, tgt, init, gate, iterations, want_corr)

    # ---- oriented surface points and point-to-line scan matching (rr_surfels.hip); any context with a config, mesh or not
    @staticmethod
    def surfels_scratch_bytes(n_frames, cfg):
        """rr_surfels_scratch_bytes: the bytes of scratch rr_surface_points_device needs for n_frames clouds under cfg"""
        g = _surfel_cfg(cfg)
        return int(lib().rr_surfels_scratch_bytes(_frames_arg(n_frames), C.byref(g)))

    def surface_points_device(self, d_points_ptr, d_offsets_ptr, n_frames, max_points, cfg, d_surfels_ptr, max_surfels, d_counts_ptr, d_scratch_ptr,
                              scratch_bytes, stream=None):
        """rr_surface_points_device on raw device addresses: the points [n_frames][max_points] and offsets [n_frames][n_angles + 1]
        rr_detect_device wrote -> SURFEL_DTYPE records [n_frames][max_surfels] in ascending cell order (None iff max_surfels is 0) and counts
        uint32 [n_frames][2] = (kept, flags).  The scratch (surfels_scratch_bytes, 16-byte aligned like the records) is the caller's; nothing
        of the context is used, so the call may run on any stream.  Every argument is checked here first."""
        self._polar_shape()
        g, n = _surfel_cfg(cfg), _frames_arg(n_frames)
        mp, ms = _int_in(max_points, 0, ICP_MAX_POINTS, "max_points"), _int_in(max_surfels, 0, SURFELS_MAX_RECORDS, "max_surfels")
        if not (d_offsets_ptr and d_counts_ptr and d_scratch_ptr) or (mp > 0 and not d_points_ptr):
            raise ValueError("surface_points_device needs point, offset, count and scratch buffers")
        if bool(d_surfels_ptr) != (ms > 0):
            raise ValueError("the records come with max_surfels > 0 and only with it")
        if (d_surfels_ptr or 0) % 16 or d_scratch_ptr % 16 or d_counts_ptr % 4:
            raise ValueError("the records and the scratch must be 16-byte aligned, the counts 4-byte aligned")
        need = self.surfels_scratch_bytes(n, g)
        if isinstance(scratch_bytes, bool) or not isinstance(scratch_bytes, (int, np.integer)) or scratch_bytes < need:
            raise ValueError("scratch of %r bytes, the call needs %d" % (scratch_bytes, need))
        self._ck(self._L.rr_surface_points_device(self._h, d_points_ptr, d_offsets_ptr, n, mp, C.byref(g), d_surfels_ptr, ms, d_counts_ptr,
                                                  d_scratch_ptr, int(scratch_bytes), stream))

    def surface_points(self, points_list, offsets, cfg, max_surfels=4096):
        """rr_surface_points on what detect() (or compensate_points()) returned: a list of n POINT_DTYPE arrays and offsets uint32
        [n][n_angles + 1] -> (a list with one SURFEL_DTYPE array per cloud: its first min(kept, max_surfels) surface points in ascending
        cell order, counts uint32 [n][2] = (kept, flags))"""
        _, n_angles = self._polar_shape()
        g, ms = _surfel_cfg(cfg), _int_in(max_surfels, 0, SURFELS_MAX_RECORDS, "max_surfels")
        buf, offs, _ = _clouds(points_list, offsets, n_angles, True)
        n, mp = buf.shape
        recs = np.zeros((n, ms), SURFEL_DTYPE) if ms else None
        counts = np.zeros((n, 2), np.uint32)
        self._ck(self._L.rr_surface_points(self._h, buf.ctypes.data, offs.ctypes.data, n, mp, C.byref(g), _ptr(recs), ms, counts.ctypes.data))
        return [recs[f, :min(int(counts[f, 0]), ms)].copy() if ms else np.zeros(0, SURFEL_DTYPE) for f in range(n)], counts

    def register_surfels_device(self, d_points_ptr, d_offsets_ptr, n_frames, max_points, d_tgt_surfels_ptr, d_tgt_count_ptr, max_tgt, d_recs_ptr,
                                d_init_ptr=None, gate=1.0, iterations=10, d_corr_ptr=None, stream=None):
        """rr_register_surfels_device: register_points_device with SURFEL_DTYPE records [max_tgt] (16-byte aligned) as the target, whose
        count is the uint32 at d_tgt_count_ptr (&counts[g][0] of surface_points_device): point-to-line ICP"""
        self._register_device("register_surfels_device", 16, d_points_ptr, d_offsets_ptr, n_frames, max_points,
                              d_tgt_surfels_ptr, d_tgt_count_ptr, max_tgt, d_recs_ptr, d_init_ptr, gate, iterations, d_corr_ptr, stream)

    def register_surfels(self, points_list, offsets, target_surfels, init=None, gate=1.0, iterations=10, want_corr=False):
        """rr_register_surfels: register_points with ONE SURFEL_DTYPE array (what surface_points returned for the target cloud) as the
        target and a point-to-line residual.  Returns ICP_DTYPE [n] (sse in (1/65536 m)^2); with want_corr also the matched surfel index
        per point, ICP_NONE for an unmatched point."""
        _, n_angles = self._polar_shape()
        pts = _cloud_list(points_list)
        tgt = np.asarray(target_surfels)
        if tgt.dtype != SURFEL_DTYPE or tgt.ndim != 1 or len(tgt) > ICP_MAX_POINTS:
            raise ValueError("the target must be a one-dimensional SURFEL_DTYPE array of at most %d records" % ICP_MAX_POINTS)
        tgt = np.ascontiguousarray(tgt)
        return self._register("register_surfels", pts, offsets, n_angles, tgt, init, gate, iterations, want_corr)

    # ---- pose-graph optimisation (rr_graph.hip); any context, with a config or not
    @staticmethod
    def graph_plan_bytes(n_nodes, n_edges):
        """rr_graph_plan_bytes: the bytes of the incidence plan of a graph of n_nodes nodes and n_edges edges"""
        n, e = _graph_shape(n_nodes, n_edges)
        return int(lib().rr_graph_plan_bytes(n, e))

    @staticmethod
    def graph_scratch_bytes(n_nodes, n_edges, cfg):
        """rr_graph_scratch_bytes: the bytes of scratch rr_optimize_graph_device needs under cfg"""
        n, e = _graph_shape(n_nodes, n_edges)
        g = _graph_cfg(cfg)
        return int(lib().rr_graph_scratch_bytes(n, e, C.byref(g)))

    def graph_plan_device(self, d_edges_ptr, n_nodes, n_edges, d_plan_ptr, plan_bytes, stream=None):
        """rr_graph_plan_device on raw device addresses: GRAPH_EDGE_DTYPE records [n_edges] (None iff n_edges is 0) -> the incidence plan
        (graph_plan_bytes, 16-byte aligned like the edges), every byte of it written.  Every argument is checked here first."""
        n, e = _graph_shape(n_nodes, n_edges)
        if not d_plan_ptr or (e > 0 and not d_edges_ptr):
            raise ValueError("graph_plan_device needs edge and plan buffers")
        if (d_edges_ptr or 0) % 16 or d_plan_ptr % 16:
            raise ValueError("the edges and the plan must be 16-byte aligned")
        need = self.graph_plan_bytes(n, e)
        if isinstance(plan_bytes, bool) or not isinstance(plan_bytes, (int, np.integer)) or plan_bytes < need:
            raise ValueError("plan of %r bytes, the call needs %d" % (plan_bytes, need))
        self._ck(self._L.rr_graph_plan_device(self._h, d_edges_ptr, n, e, d_plan_ptr, int(plan_bytes), stream))

    def graph_plan(self, edges, n_nodes):
        """rr_graph_plan: GRAPH_EDGE_DTYPE [E] (native.graph_edges makes them) and the node count -> the incidence plan as uint8 bytes: every
        node's edges in ascending edge index.  It depends on the endpoints alone and serves any number of optimize_graph calls."""
        e = _graph_edges_arg(edges)
        n, ne = _graph_shape(n_nodes, len(e))
        plan = np.zeros(self.graph_plan_bytes(n, ne), np.uint8)
        self._ck(self._L.rr_graph_plan(self._h, e.ctypes.data if ne else None, n, ne, plan.ctypes.data, plan.nbytes))
        return plan

    def optimize_graph_device(self, d_states_ptr, d_fixed_ptr, d_edges_ptr, n_nodes, n_edges, d_plan_ptr, cfg, d_recs_ptr, d_scratch_ptr, scratch_bytes,
                              d_edge_flags_ptr=None, stream=None):
        """rr_optimize_graph_device on raw device addresses: float64 states [n_nodes][4] in and out, a fixed byte per node, the edges, their
        plan -> GRAPH_REC_DTYPE [iterations + 1] and, if asked for, a flag byte per edge.  The scratch (graph_scratch_bytes) is the caller's;
        nothing of the context is used, so the call may run on any stream.  Every argument is checked here first."""
        n, e = _graph_shape(n_nodes, n_edges)
        g = _graph_cfg(cfg)
        if not (d_states_ptr and d_fixed_ptr and d_plan_ptr and d_recs_ptr and d_scratch_ptr) or (e > 0 and not d_edges_ptr):
            raise ValueError("optimize_graph_device needs state, fixed, edge, plan, record and scratch buffers")
        if d_states_ptr % 16 or (d_edges_ptr or 0) % 16 or d_plan_ptr % 16 or d_recs_ptr % 16 or d_scratch_ptr % 16:
            raise ValueError("the states, the edges, the plan, the records and the scratch must be 16-byte aligned")
        need = self.graph_scratch_bytes(n, e, g)
        if isinstance(scratch_bytes, bool) or not isinstance(scratch_bytes, (int, np.integer)) or scratch_bytes < need:
            raise ValueError("scratch of %r bytes, the call needs %d" % (scratch_bytes, need))
        self._ck(self._L.rr_optimize_graph_device(self._h, d_states_ptr, d_fixed_ptr, d_edges_ptr, n, e, d_plan_ptr, C.byref(g), d_recs_ptr,
                                                  d_edge_flags_ptr, d_scratch_ptr, int(scratch_bytes), stream))

    def optimize_graph(self, states, fixed, edges, cfg, plan=None, want_flags=False):
        """rr_optimize_graph: float64 states [N][4] = (c, s, tx, ty) (native.se2_states), a fixed flag per node, GRAPH_EDGE_DTYPE edges and a
        graph_config (or a dict of its arguments) -> (the optimised states, GRAPH_REC_DTYPE [iterations + 1]); with want_flags also the flag
        byte per edge of the last linearisation.  plan: what graph_plan returned for these endpoints, or None to build it here."""
        x = np.array(states, np.float64, order="C")
        if x.ndim != 2 or x.shape[1] != 4:
            raise ValueError("states must have shape [n][4], got %s" % (x.shape,))
        e = _graph_edges_arg(edges)
        n, ne = _graph_shape(len(x), len(e))
        fx = np.ascontiguousarray(np.asarray(fixed) != 0, np.uint8)
        if fx.shape != (n,):
            raise ValueError("one fixed flag per node, got shape %s" % (fx.shape,))
        g = _graph_cfg(cfg)
        if plan is None:
            plan = self.graph_plan(e, n)
        plan = np.asarray(plan)
        if plan.dtype != np.uint8 or plan.ndim != 1 or plan.nbytes < self.graph_plan_bytes(n, ne):
            raise ValueError("the plan must be the uint8 bytes graph_plan returned for this graph")
        plan = np.ascontiguousarray(plan)
        recs = np.zeros(g.iterations + 1, GRAPH_REC_DTYPE)
        flags = np.zeros(ne, np.uint8) if want_flags else None
        self._ck(self._L.rr_optimize_graph(self._h, x.ctypes.data, fx.ctypes.data, e.ctypes.data if ne else None, n, ne, plan.ctypes.data, C.byref(g),
                                           recs.ctypes.data, _ptr(flags) if ne else None))
        return (x, recs, flags) if want_flags else (x, recs)

    # ---- likelihood field (rr_field.hip): clouds into an occupancy grid, its exact distance transform, pose hypotheses scored against it
    def rasterize_points_device(self, d_points_ptr, d_offsets_ptr, n_frames, max_points, field_cfg, d_occ_ptr, d_states_ptr=None, stream=None):
        """rr_rasterize_points_device: ones into the uint8 grid [height][width] at d_occ_ptr (zeroed by the caller, or holding earlier
        clouds) for the points [n_frames][max_points] and offsets [n_frames][n_angles + 1] rr_detect_device wrote; d_states_ptr: float64
        [n_frames][4] = (c, s, tx, ty), each frame into the map frame, or None (identity); on `stream`"""
        self._polar_shape()
        n, mp, g = _frames_arg(n_frames), _int_in(max_points, 0, ICP_MAX_POINTS, "max_points"), _field_cfg(field_cfg)
        if not d_offsets_ptr or not d_occ_ptr or (mp > 0 and not d_points_ptr):
            raise ValueError("rasterize_points_device needs point, offset and grid buffers")
        self._ck(self._L.rr_rasterize_points_device(self._h, d_points_ptr, d_offsets_ptr, n, mp, d_states_ptr, C.byref(g), d_occ_ptr, stream))

    def rasterize_points(self, points_list, offsets, field_cfg, states=None, occ=None):
        """rr_rasterize_points on what detect() (or compensate_points()) returned: a list of n POINT_DTYPE arrays and offsets uint32
        [n][n_angles + 1]; states float64 [n][4] (se2_states makes them) or None; occ: a uint8 [height][width] grid to accumulate into
        (it is not modified) or None for an empty one.  Returns the grid."""
        g = _field_cfg(field_cfg)
        buf, offs, st = self._posed_clouds(points_list, offsets, states)
        out = self._field_grid(occ, g, np.uint8, "occ").copy() if occ is not None else np.zeros((g.height, g.width), np.uint8)
        self._ck(self._L.rr_rasterize_points(self._h, buf.ctypes.data, offs.ctypes.data, len(buf), buf.shape[1], _ptr(st), C.byref(g),
                                             out.ctypes.data))
        return out

    def _posed_clouds(self, points_list, offsets, states):
        """what the rasteriser and the occupancy update take from detect() (or compensate_points()): a list of n POINT_DTYPE arrays, offsets
        uint32 [n][n_angles + 1] and states float64 [n][4] or None -> (the points as one POINT_DTYPE [n][max_points] block, the offsets,
        the states), all contiguous"""
        _, n_angles = self._polar_shape()
        buf, offs, _ = _clouds(points_list, offsets, n_angles, True)
        return buf, offs, None if states is None else _states(states, np.float64, "states", n=len(buf))

    @staticmethod
    def _field_grid(a, g, dtype, what):
        x = np.asarray(a)
        if x.dtype != dtype or x.shape != (g.height, g.width):
            raise ValueError("%s must be %s [%d][%d], got %s %s" % (what, np.dtype(dtype).name, g.height, g.width, x.dtype, x.shape))
        return np.ascontiguousarray(x)

    def distance_field_device(self, d_occ_ptr, field_cfg, d_field_ptr, threshold=1, stream=None):
        """rr_distance_field_device: the uint16 field [height][width] at d_field_ptr from the uint8 grid at d_occ_ptr (occupied: >= threshold)"""
        g, th = _field_cfg(field_cfg), _int_in(threshold, 1, 255, "threshold")
        if not d_occ_ptr or not d_field_ptr or d_occ_ptr == d_field_ptr:
            raise ValueError("distance_field_device needs a grid and a field buffer that do not alias")
        self._ck(self._L.rr_distance_field_device(self._h, d_occ_ptr, th, C.byref(g), d_field_ptr, stream))

    def distance_field(self, occ, field_cfg, threshold=1):
        """rr_distance_field: uint8 [height][width] (occupied: >= threshold) -> uint16 [height][width], min(max_dist^2, the exact squared
        distance in cells to the nearest occupied cell)"""
        g, th = _field_cfg(field_cfg), _int_in(threshold, 1, 255, "threshold")
        x = self._field_grid(occ, g, np.uint8, "occ")
        out = np.zeros((g.height, g.width), np.uint16)
        self._ck(self._L.rr_distance_field(self._h, x.ctypes.data, th, C.byref(g), out.ctypes.data))
        return out

    def score_poses_device(self, d_points_ptr, d_count_ptr, max_points, d_states_ptr, n_hyp, d_field_ptr, field_cfg, d_recs_ptr, stream=None):
        """rr_score_poses_device: FIELD_DTYPE records [n_hyp] in HBM for the float32 states [n_hyp][4] = (c, s, tx, ty), each the scan's
        sensor frame into the map frame, of ONE scan: the points at d_points_ptr whose count is the uint32 at d_count_ptr; on `stream`"""
        mp, n, g = _int_in(max_points, 0, ICP_MAX_POINTS, "max_points"), _int_in(n_hyp, 1, FIELD_MAX_HYP, "n_hyp"), _field_cfg(field_cfg)
        if not d_count_ptr or not d_states_ptr or not d_field_ptr or not d_recs_ptr or (mp > 0 and not d_points_ptr):
            raise ValueError("score_poses_device needs point, count, state, field and record buffers")
        self._ck(self._L.rr_score_poses_device(self._h, d_points_ptr, d_count_ptr, mp, d_states_ptr, n, d_field_ptr, C.byref(g), d_recs_ptr, stream))

    def score_poses(self, points, states, field, field_cfg):
        """rr_score_poses: one POINT_DTYPE cloud, float32 states [n][4] (pose_lattice makes them), the uint16 field of distance_field ->
        FIELD_DTYPE [n]; lower sum_d2 is better"""
        g = _field_cfg(field_cfg)
        p = _scan(points, 0, "the scan")
        st = _states(states, np.float32, "states", FIELD_MAX_HYP)
        f = self._field_grid(field, g, np.uint16, "field")
        recs = np.zeros(len(st), FIELD_DTYPE)
        self._ck(self._L.rr_score_poses(self._h, p.ctypes.data if len(p) else None, len(p), len(p), st.ctypes.data, len(st), f.ctypes.data,
                                        C.byref(g), recs.ctypes.data))
        return recs

    # ---- occupancy mapping (rr_occupancy.hip): posed scans fused into an int32 evidence grid, and its uint8 map
    def _occ_cfg(self, occ_cfg):
        """an RROccupancyConfig or a dict of occupancy_config's arguments, held to this context's n_cells"""
        n_cells, _ = self._polar_shape()
        if isinstance(occ_cfg, RROccupancyConfig):
            return occupancy_config(occ_cfg.l_hit, occ_cfg.l_free, occ_cfg.margin_bins, occ_cfg.max_free_bin, n_cells)
        if isinstance(occ_cfg, dict):
            return occupancy_config(n_cells=n_cells, **occ_cfg)
        raise ValueError("an occupancy config must be an RROccupancyConfig (native.occupancy_config makes one) or a dict of its arguments, got %r"
                         % (occ_cfg,))

    def occupancy_update_device(self, d_points_ptr, d_offsets_ptr, n_frames, max_points, field_cfg, occ_cfg, d_profile_ptr, d_evidence_ptr,
                                d_states_ptr=None, stream=None):
        """rr_occupancy_update_device: the points [n_frames][max_points] and offsets [n_frames][n_angles + 1] rr_detect_device wrote, fused
        into the int32 evidence [height][width] at d_evidence_ptr (zeroed by the caller, or holding earlier scans); d_profile_ptr: float32
        [n_frames][n_angles] the call writes; d_states_ptr: float64 [n_frames][4] = (c, s, tx, ty), each scan's sensor frame into the map
        frame, or None (identity); on `stream`"""
        o = self._occ_cfg(occ_cfg)
        n, mp, g = _frames_arg(n_frames), _int_in(max_points, 0, ICP_MAX_POINTS, "max_points"), _grid_cfg(field_cfg)
        if not d_offsets_ptr or not d_profile_ptr or not d_evidence_ptr or (mp > 0 and not d_points_ptr):
            raise ValueError("occupancy_update_device needs point, offset, profile and evidence buffers")
        self._ck(self._L.rr_occupancy_update_device(self._h, d_points_ptr, d_offsets_ptr, n, mp, d_states_ptr, C.byref(g), C.byref(o), d_profile_ptr,
                                                    d_evidence_ptr, stream))

    def occupancy_update(self, points_list, offsets, field_cfg, occ_cfg, states=None, evidence=None):
        """rr_occupancy_update on what detect() (or compensate_points()) returned: a list of n POINT_DTYPE arrays and offsets uint32
        [n][n_angles + 1]; states float64 [n][4] (se2_states makes them), each scan's sensor frame into the map frame, or None; evidence: an
        int32 [height][width] grid to accumulate into (it is not modified) or None for an empty one.  Returns the evidence."""
        g, o = _grid_cfg(field_cfg), self._occ_cfg(occ_cfg)
        buf, offs, st = self._posed_clouds(points_list, offsets, states)
        out = self._field_grid(evidence, g, np.int32, "evidence").copy() if evidence is not None else np.zeros((g.height, g.width), np.int32)
        self._ck(self._L.rr_occupancy_update(self._h, buf.ctypes.data, offs.ctypes.data, len(buf), buf.shape[1], _ptr(st), C.byref(g), C.byref(o),
                                             out.ctypes.data))
        return out

    def occupancy_map_device(self, d_evidence_ptr, field_cfg, d_occ_ptr, stream=None):
        """rr_occupancy_map_device: the uint8 map [height][width] at d_occ_ptr = clamp(128 + evidence, 0, 255) of the int32 evidence"""
        g = _grid_cfg(field_cfg)
        if not d_evidence_ptr or not d_occ_ptr:
            raise ValueError("occupancy_map_device needs an evidence and a map buffer")
        self._ck(self._L.rr_occupancy_map_device(self._h, d_evidence_ptr, C.byref(g), d_occ_ptr, stream))

    def occupancy_map(self, evidence, field_cfg):
        """rr_occupancy_map: int32 [height][width] -> uint8 [height][width]: 128 unknown, below it free, above it occupied
        (distance_field(map, cfg, threshold=129) takes it as it is)"""
        g = _grid_cfg(field_cfg)
        ev = self._field_grid(evidence, g, np.int32, "evidence")
        out = np.zeros((g.height, g.width), np.uint8)
        self._ck(self._L.rr_occupancy_map(self._h, ev.ctypes.data, C.byref(g), out.ctypes.data))
        return out

    # ---- particle filter step (rr_filter.hip): records -> weights -> systematic resampling -> odometry plus diffusion
    def filter_resample_device(self, d_recs_ptr, n, d_table_ptr, n_out, filter_cfg, d_cum_ptr, d_ancestors_ptr, d_summary_ptr, stream=None):
        """rr_filter_resample_device: the FIELD_DTYPE records [n] score_poses_device wrote and the uint16 weight table [n_table] at
        d_table_ptr -> the inclusive sums uint64 [n] at d_cum_ptr, the ancestors uint32 [n_out] and one FILTER_SUMMARY_DTYPE record; on
        `stream`"""
        f = _filter_cfg(filter_cfg)
        n, m = _int_in(n, 1, FILTER_MAX_N, "n"), _int_in(n_out, 1, FILTER_MAX_N, "n_out")
        if not d_recs_ptr or not d_table_ptr or not d_cum_ptr or not d_ancestors_ptr or not d_summary_ptr:
            raise ValueError("filter_resample_device needs record, table, cum, ancestor and summary buffers")
        self._ck(self._L.rr_filter_resample_device(self._h, d_recs_ptr, n, d_table_ptr, m, C.byref(f), d_cum_ptr, d_ancestors_ptr, d_summary_ptr,
                                                   stream))

    def filter_resample(self, recs, table, n_out, filter_cfg):
        """rr_filter_resample: FIELD_DTYPE records [n] (score_poses returns them) and the uint16 table of filter_weight_table ->
        (cum uint64 [n], ancestors uint32 [n_out], the FILTER_SUMMARY_DTYPE record)"""
        f = _filter_cfg(filter_cfg)
        r, t = np.asarray(recs), np.asarray(table)
        if r.dtype != FIELD_DTYPE or r.ndim != 1 or not 1 <= len(r) <= FILTER_MAX_N:
            raise ValueError("recs must be a one-dimensional FIELD_DTYPE array of 1..%d records" % FILTER_MAX_N)
        if t.dtype != np.uint16 or t.shape != (f.n_table,):
            raise ValueError("the table must be uint16 [n_table = %d], got %s %s" % (f.n_table, t.dtype, t.shape))
        m = _int_in(n_out, 1, FILTER_MAX_N, "n_out")
        r, t = np.ascontiguousarray(r), np.ascontiguousarray(t)
        cum, anc, summary = np.zeros(len(r), np.uint64), np.zeros(m, np.uint32), np.zeros(1, FILTER_SUMMARY_DTYPE)
        self._ck(self._L.rr_filter_resample(self._h, r.ctypes.data, len(r), t.ctypes.data, m, C.byref(f), cum.ctypes.data, anc.ctypes.data,
                                            summary.ctypes.data))
        return cum, anc, summary[0]

    def filter_move_device(self, d_states_in_ptr, n, d_ancestors_ptr, n_out, increment, filter_cfg, d_states_out_ptr, stream=None):
        """rr_filter_move_device: float32 states [n][4] = (c, s, tx, ty) in HBM, gathered through the uint32 ancestors [n_out] (None: draw j
        takes state j), moved by the increment (Dc, Ds, dx, dy) in the sensor frame (None: the identity) plus the config's diffusion,
        into the float32 [n_out][4] at d_states_out_ptr, which must not overlap the input; on `stream`"""
        f, inc = _filter_cfg(filter_cfg), _increment(increment)
        n, m = _int_in(n, 1, FILTER_MAX_N, "n"), _int_in(n_out, 1, FILTER_MAX_N, "n_out")
        if not d_states_in_ptr or not d_states_out_ptr:
            raise ValueError("filter_move_device needs both state buffers")
        if not d_ancestors_ptr and m > n:
            raise ValueError("n_out (%d) must not exceed n (%d) without ancestors" % (m, n))
        self._ck(self._L.rr_filter_move_device(self._h, d_states_in_ptr, n, d_ancestors_ptr, m, *inc, C.byref(f), d_states_out_ptr, stream))

    def filter_move(self, states, ancestors, increment, filter_cfg):
        """rr_filter_move: float32 states [n][4], uint32 ancestors [n_out] or None (every state once), the increment (Dc, Ds, dx, dy) or None
        -> the moved states float32 [n_out][4]"""
        f, inc = _filter_cfg(filter_cfg), _increment(increment)
        st = _states(states, np.float32, "states", FILTER_MAX_N)
        anc = None
        if ancestors is not None:
            anc = np.asarray(ancestors)
            if anc.dtype.kind not in "iu" or anc.ndim != 1 or not 1 <= len(anc) <= FILTER_MAX_N or anc.min() < 0 or anc.max() >= len(st):
                raise ValueError("ancestors must be integers in [0, %d) of shape [n_out], n_out in 1..%d" % (len(st), FILTER_MAX_N))
            anc = np.ascontiguousarray(anc, np.uint32)
        m = len(st) if anc is None else len(anc)
        out = np.zeros((m, 4), np.float32)
        self._ck(self._L.rr_filter_move(self._h, st.ctypes.data, len(st), _ptr(anc), m, *inc, C.byref(f), out.ctypes.data))
        return out

    # ---- map refinement (rr_refine.hip): the nearest-cell transform of a grid map, and ICP of one scan against it from many states
    def nearest_field_device(self, d_occ_ptr, field_cfg, d_nearest_ptr, threshold=1, stream=None):
        """rr_nearest_field_device: the uint32 table [height][width] at d_nearest_ptr from the uint8 grid at d_occ_ptr (occupied: >=
        threshold): per cell the linear index of the nearest occupied cell, NEAREST_NONE where none lies within max_dist"""
        g, th = _field_cfg(field_cfg), _int_in(threshold, 1, 255, "threshold")
        if not d_occ_ptr or not d_nearest_ptr or d_occ_ptr == d_nearest_ptr:
            raise ValueError("nearest_field_device needs a grid and a table buffer that do not alias")
        self._ck(self._L.rr_nearest_field_device(self._h, d_occ_ptr, th, C.byref(g), d_nearest_ptr, stream))

    def nearest_field(self, occ, field_cfg, threshold=1):
        """rr_nearest_field: uint8 [height][width] (occupied: >= threshold) -> uint32 [height][width]: jy * width + jx of the nearest occupied
        cell (ties to the lowest index), NEAREST_NONE where its squared distance is not below max_dist^2"""
        g, th = _field_cfg(field_cfg), _int_in(threshold, 1, 255, "threshold")
        x = self._field_grid(occ, g, np.uint8, "occ")
        out = np.zeros((g.height, g.width), np.uint32)
        self._ck(self._L.rr_nearest_field(self._h, x.ctypes.data, th, C.byref(g), out.ctypes.data))
        return out

    def refine_poses_device(self, d_points_ptr, d_count_ptr, max_points, d_init_ptr, n_hyp, d_nearest_ptr, field_cfg, d_recs_ptr, iterations=10,
                            stream=None):
        """rr_refine_poses_device: ICP_DTYPE records [n_hyp] in HBM from the float64 initial states [n_hyp][4] = (c, s, tx, ty), each the
        scan's sensor frame into the map frame, of ONE scan: the points at d_points_ptr whose count is the uint32 at d_count_ptr, against the
        uint32 table of nearest_field_device; one launch on `stream`"""
        mp, n, g = _int_in(max_points, 0, ICP_MAX_POINTS, "max_points"), _int_in(n_hyp, 1, FIELD_MAX_HYP, "n_hyp"), _refine_cfg(field_cfg)
        it = _int_in(iterations, 0, 64, "iterations")
        if not d_count_ptr or not d_init_ptr or not d_nearest_ptr or not d_recs_ptr or (mp > 0 and not d_points_ptr):
            raise ValueError("refine_poses_device needs point, count, state, table and record buffers")
        self._ck(self._L.rr_refine_poses_device(self._h, d_points_ptr, d_count_ptr, mp, d_init_ptr, n, d_nearest_ptr, C.byref(g), it, d_recs_ptr,
                                                stream))

    def refine_poses(self, points, init, nearest, field_cfg, iterations=10):
        """rr_refine_poses: one POINT_DTYPE cloud, initial states [n][4] = (c, s, tx, ty) (se2_states, pose_lattice or a filter's states; they
        are widened to float64 and normalised by the library), the uint32 table of nearest_field -> ICP_DTYPE [n]: the refined state, sse,
        n_matched and flags of the last pass; iterations 0..64 (0 scores the states as they stand)"""
        g, it = _refine_cfg(field_cfg), _int_in(iterations, 0, 64, "iterations")
        p = _scan(points, 0, "the scan")
        st = _states(init, np.float64, "init", FIELD_MAX_HYP)
        nr = self._field_grid(nearest, g, np.uint32, "nearest")
        recs = np.zeros(len(st), ICP_DTYPE)
        self._ck(self._L.rr_refine_poses(self._h, p.ctypes.data if len(p) else None, len(p), len(p), st.ctypes.data, len(st), nr.ctypes.data,
                                         C.byref(g), it, recs.ctypes.data))
        return recs

    # ---- mesh maps (rr_slice.hip): the context's posed triangles sliced into the grid map
    def _skip_bytes(self, skip_objects):
        """object ids to leave out (or None / empty: none) -> uint8 [n_objects] or None"""
        if skip_objects is None:
            return None
        ids = np.asarray(list(skip_objects))
        if ids.size == 0:
            return None
        n = int(getattr(self, "n_objects", 1))
        if ids.dtype.kind not in "iu" or ids.ndim != 1 or ids.min() < 0 or ids.max() >= n:
            raise ValueError("skip_objects must be object ids in 0..%d, got %r" % (n - 1, skip_objects))
        skip = np.zeros(n, np.uint8)
        skip[ids] = 1
        return skip

    def slice_mesh_device(self, slice_cfg, field_cfg, d_occ_ptr, d_object_ptr=None, d_skip_ptr=None, stream=None):
        """rr_slice_mesh_device: a 1 into every cell of the uint8 grid [height][width] at d_occ_ptr that a posed triangle touches inside the
        band; with d_object_ptr the smallest object id per cell into that uint32 plane (filled with OBJECT_NONE by the caller); d_skip_ptr
        uint8 [n_objects], non-zero: the object is left out.  Enqueued on `stream`; the caller orders it against the scene setters"""
        sc, g = _slice_cfg(slice_cfg), _field_cfg(field_cfg)
        if not d_occ_ptr or (d_object_ptr and d_object_ptr % 4):
            raise ValueError("slice_mesh_device needs a grid buffer, and a 4-byte aligned object plane if one is given")
        self._ck(self._L.rr_slice_mesh_device(self._h, C.byref(sc), C.byref(g), d_skip_ptr, d_occ_ptr, d_object_ptr, stream))

    def slice_mesh(self, slice_cfg, field_cfg, skip_objects=None, with_objects=False, occ=None, objects=None):
        """rr_slice_mesh: the scene's triangles inside the band -> uint8 [height][width] of zeros and ones, accumulated into a copy of `occ`
        when one is given; with_objects (or `objects`, a plane to lower): also the uint32 plane of the smallest object id per cell,
        OBJECT_NONE where nothing marks it.  skip_objects: object ids to leave out.  Returns occ or (occ, objects)"""
        sc, g = _slice_cfg(slice_cfg), _field_cfg(field_cfg)
        skip = self._skip_bytes(skip_objects)
        out = np.zeros((g.height, g.width), np.uint8) if occ is None else self._field_grid(occ, g, np.uint8, "occ").copy()
        obj = None
        if objects is not None:
            obj = self._field_grid(objects, g, np.uint32, "objects").copy()
        elif with_objects:
            obj = np.full((g.height, g.width), OBJECT_NONE, np.uint32)
        self._ck(self._L.rr_slice_mesh(self._h, C.byref(sc), C.byref(g), _ptr(skip), out.ctypes.data, _ptr(obj)))
        return out if obj is None else (out, obj)

    # ---- connected components (rr_components.hip): thresholded uint8 planes -> label planes, cleaned planes, one record per component
    @staticmethod
    def _component_planes(planes, g):
        """uint8 [n][height][width] (or one plane) -> contiguous [n][height][width], n in 1..65535"""
        x = np.asarray(planes)
        if x.dtype != np.uint8 or x.ndim not in (2, 3) or x.shape[-2:] != (g.height, g.width):
            raise ValueError("planes must be uint8 [n][%d][%d] or one such plane, got %s %s" % (g.height, g.width, x.dtype, x.shape))
        x = np.ascontiguousarray(x).reshape(-1, g.height, g.width)
        if not 1 <= len(x) <= COMPONENTS_MAX_PLANES:
            raise ValueError("1..%d planes, got %d" % (COMPONENTS_MAX_PLANES, len(x)))
        return x

    @staticmethod
    def components_scratch_bytes(n_planes, cfg):
        """rr_components_scratch_bytes: the bytes of scratch rr_label_components_device needs for n_planes planes of cfg's shape"""
        g = _components_cfg(cfg)
        return int(lib().rr_components_scratch_bytes(_int_in(n_planes, 1, COMPONENTS_MAX_PLANES, "n_planes"), C.byref(g)))

    def label_components_device(self, d_planes_ptr, n_planes, cfg, d_labels_ptr, d_clean_ptr, d_comps_ptr, d_counts_ptr, d_scratch_ptr, scratch_bytes,
                                stream=None):
        """rr_label_components_device on raw device addresses: uint8 planes [n][H][W] -> labels uint32 [n][H][W] (or None), the cleaned planes
        uint8 [n][H][W] (or None, never overlapping the input), COMPONENT_DTYPE records [n][max_components] (None iff max_components is 0)
        and counts uint32 [n][2] = (kept, dropped).  The scratch (components_scratch_bytes, 16-byte aligned like the records) is the
        caller's; nothing of the context is used, so the call may run on any stream.  Every argument is checked here first."""
        g, n = _components_cfg(cfg), _int_in(n_planes, 1, COMPONENTS_MAX_PLANES, "n_planes")
        if not (d_planes_ptr and d_counts_ptr and d_scratch_ptr):
            raise ValueError("label_components_device needs plane, count and scratch buffers")
        if bool(d_comps_ptr) != (g.max_components > 0):
            raise ValueError("the records come with max_components > 0 and only with it")
        if (d_comps_ptr or 0) % 16 or d_scratch_ptr % 16 or (d_labels_ptr or 0) % 4 or d_counts_ptr % 4:
            raise ValueError("the records and the scratch must be 16-byte aligned, the label plane and the counts 4-byte aligned")
        nbytes = n * g.height * g.width
        if d_clean_ptr and d_planes_ptr < d_clean_ptr + nbytes and d_clean_ptr < d_planes_ptr + nbytes:
            raise ValueError("the cleaned planes must not overlap the input")
        need = self.components_scratch_bytes(n, g)
        if isinstance(scratch_bytes, bool) or not isinstance(scratch_bytes, (int, np.integer)) or scratch_bytes < need:
            raise ValueError("scratch of %r bytes, the call needs %d" % (scratch_bytes, need))
        self._ck(self._L.rr_label_components_device(self._h, d_planes_ptr, n, C.byref(g), d_labels_ptr, d_clean_ptr, d_comps_ptr, d_counts_ptr,
                                                    d_scratch_ptr, int(scratch_bytes), stream))

    def label_components_tensors(self, d_planes, cfg, labels=True, clean=False, stream=None):
        """the device form on a torch uint8 tensor [n][H][W] (or [H][W]) of this context's device: allocates the outputs and sizes and owns
        the scratch as a torch byte tensor, enqueues on `stream` (a raw handle; None: the context's own stream) and returns a dict of tensors
        that stay in HBM: labels int32 [n][H][W] (the words are uint32, LABEL_NONE reads -1) and clean uint8 [n][H][W] as asked for, comps
        uint8 [n][max_components * 80] (component_records views them on the host), counts int32 [n][2], and the scratch, which the caller keeps
        alive until the stream has passed the call"""
        import torch
        g = _components_cfg(cfg)
        if not isinstance(d_planes, torch.Tensor) or d_planes.dtype != torch.uint8 or d_planes.dim() not in (2, 3) or \
                tuple(d_planes.shape[-2:]) != (g.height, g.width) or not d_planes.is_cuda or not d_planes.is_contiguous():
            raise ValueError("planes must be a contiguous uint8 tensor [n][%d][%d] on the device" % (g.height, g.width))
        n = 1 if d_planes.dim() == 2 else int(d_planes.shape[0])
        dev = d_planes.device
        out = {"counts": torch.empty((n, 2), dtype=torch.int32, device=dev)}
        if labels:
            out["labels"] = torch.empty((n, g.height, g.width), dtype=torch.int32, device=dev)
        if clean:
            out["clean"] = torch.empty((n, g.height, g.width), dtype=torch.uint8, device=dev)
        if g.max_components:
            out["comps"] = torch.empty((n, g.max_components * COMPONENT_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        nbytes = self.components_scratch_bytes(n, g)
        out["scratch"] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ptr = lambda k: out[k].data_ptr() if k in out else None      # noqa: E731
        self.label_components_device(d_planes.data_ptr(), n, g, ptr("labels"), ptr("clean"), ptr("comps"), ptr("counts"), ptr("scratch"), nbytes, stream)
        return out

    @staticmethod
    def component_counts(counts):
        """the counts of a call (a torch tensor on the device, or numpy) -> uint32 [n][2] = (kept, dropped) on the host"""
        c = counts.detach().cpu().numpy() if hasattr(counts, "detach") else np.asarray(counts)
        return np.ascontiguousarray(c).view(np.uint32).reshape(-1, 2)

    @staticmethod
    def component_records(comps, counts):
        """the records and counts of a call, brought home (torch tensors or numpy) -> a list with one COMPONENT_DTYPE array per plane: the
        min(kept, max_components) records that were written"""
        k = Context.component_counts(counts)
        if comps is None:
            return [np.zeros(0, COMPONENT_DTYPE) for _ in k]
        c = np.ascontiguousarray(comps.detach().cpu().numpy() if hasattr(comps, "detach") else comps).view(np.uint8).reshape(len(k), -1).view(COMPONENT_DTYPE)
        return [c[a, :min(int(k[a, 0]), c.shape[1])].copy() for a in range(len(k))]

    def label_components(self, planes, cfg, labels=True, clean=False):
        """rr_label_components on host planes uint8 [n][H][W] (or one plane): returns a dict with labels uint32 [n][H][W] (LABEL_NONE on the
        background and on dropped components) and clean uint8 [n][H][W] as asked for, comps (a list with one COMPONENT_DTYPE array per plane:
        the first min(kept, max_components) components in ascending root order) and counts uint32 [n][2] = (kept, dropped)"""
        g = _components_cfg(cfg)
        x = self._component_planes(planes, g)
        n = len(x)
        out = {"counts": np.zeros((n, 2), np.uint32)}
        if labels:
            out["labels"] = np.empty(x.shape, np.uint32)
        if clean:
            out["clean"] = np.empty(x.shape, np.uint8)
        recs = np.zeros((n, g.max_components), COMPONENT_DTYPE) if g.max_components else None
        self._ck(self._L.rr_label_components(self._h, x.ctypes.data, n, C.byref(g), _ptr(out.get("labels")), _ptr(out.get("clean")), _ptr(recs),
                                             out["counts"].ctypes.data))
        out["comps"] = self.component_records(recs, out["counts"])
        return out

    # ---- correlative scan matching (rr_correlate.hip): the min-pyramid of a field, and the exact search of a window of whole-cell offsets
    @staticmethod
    def _pyramid_planes(a, g, levels, what="pyramid"):
        """uint16 [n][height][width] with n > levels -> contiguous, its first levels + 1 planes"""
        x = np.asarray(a)
        if x.dtype != np.uint16 or x.ndim != 3 or x.shape[1:] != (g.height, g.width) or len(x) < levels + 1:
            raise ValueError("%s must be uint16 [%d or more][%d][%d], got %s %s" % (what, levels + 1, g.height, g.width, x.dtype, x.shape))
        return np.ascontiguousarray(x[:levels + 1])

    def field_pyramid_device(self, d_field_ptr, field_cfg, levels, d_pyramid_ptr, stream=None):
        """rr_field_pyramid_device: uint16 planes [levels + 1][height][width] at d_pyramid_ptr from the field at d_field_ptr, which may be the
        pyramid's own plane 0"""
        g, lv = _field_cfg(field_cfg), _int_in(levels, 0, CORR_MAX_LEVELS, "levels")
        if not d_field_ptr or not d_pyramid_ptr or d_field_ptr % 2 or d_pyramid_ptr % 2:
            raise ValueError("field_pyramid_device needs a field and a pyramid buffer, 2-byte aligned")
        self._ck(self._L.rr_field_pyramid_device(self._h, d_field_ptr, C.byref(g), lv, d_pyramid_ptr, stream))

    def field_pyramid(self, field, field_cfg, levels):
        """rr_field_pyramid: the uint16 field of distance_field -> uint16 [levels + 1][height][width]; plane 0 is the field, plane h the minimum
        over the 2^h x 2^h cells from each cell on, max_dist^2 beyond the edge"""
        g, lv = _field_cfg(field_cfg), _int_in(levels, 0, CORR_MAX_LEVELS, "levels")
        f = self._field_grid(field, g, np.uint16, "field")
        out = np.zeros((lv + 1, g.height, g.width), np.uint16)
        self._ck(self._L.rr_field_pyramid(self._h, f.ctypes.data, C.byref(g), lv, out.ctypes.data))
        return out

    @staticmethod
    def correlate_scratch_bytes(n_rot, max_points, corr_cfg):
        """rr_correlate_scratch_bytes: the bytes of scratch rr_correlate_scan_device needs"""
        n = _int_in(n_rot, 1, CORR_MAX_ROT, "n_rot")
        k = _corr_cfg(corr_cfg, n)
        return int(lib().rr_correlate_scratch_bytes(n, _int_in(max_points, 0, ICP_MAX_POINTS, "max_points"), C.byref(k)))

    def correlate_scan_device(self, d_points_ptr, d_count_ptr, max_points, d_rot_ptr, n_rot, d_pyramid_ptr, field_cfg, corr_cfg, d_rec_ptr,
                              d_scratch_ptr, scratch_bytes, stream=None):
        """rr_correlate_scan_device on raw device addresses: one CORR_DTYPE record at d_rec_ptr for ONE scan (the points at d_points_ptr whose
        count is the uint32 at d_count_ptr), the float32 anchor states [n_rot][4] = (c, s, tx, ty) and the pyramid of field_pyramid_device.
        The scratch (correlate_scratch_bytes, 16-byte aligned like the record) is the caller's; nothing of the context is used, so the call
        may run on any stream.  Every argument is checked here first."""
        mp, n, g = _int_in(max_points, 0, ICP_MAX_POINTS, "max_points"), _int_in(n_rot, 1, CORR_MAX_ROT, "n_rot"), _field_cfg(field_cfg)
        k = _corr_cfg(corr_cfg, n)
        if not (d_count_ptr and d_rot_ptr and d_pyramid_ptr and d_rec_ptr and d_scratch_ptr) or (mp > 0 and not d_points_ptr):
            raise ValueError("correlate_scan_device needs point, count, state, pyramid, record and scratch buffers")
        if d_rot_ptr % 4 or d_pyramid_ptr % 2 or d_rec_ptr % 16 or d_scratch_ptr % 16:
            raise ValueError("the states must be 4-byte, the pyramid 2-byte, the record and the scratch 16-byte aligned")
        need = self.correlate_scratch_bytes(n, mp, k)
        if isinstance(scratch_bytes, bool) or not isinstance(scratch_bytes, (int, np.integer)) or scratch_bytes < need:
            raise ValueError("scratch of %r bytes, the call needs %d" % (scratch_bytes, need))
        self._ck(self._L.rr_correlate_scan_device(self._h, d_points_ptr, d_count_ptr, mp, d_rot_ptr, n, d_pyramid_ptr, C.byref(g), C.byref(k),
                                                  d_rec_ptr, d_scratch_ptr, int(scratch_bytes), stream))

    def correlate_scan(self, points, rot_states, pyramid, field_cfg, corr_cfg):
        """rr_correlate_scan: one POINT_DTYPE cloud, float32 anchor states [n_rot][4] (se2-style (cos yaw, sin yaw, x, y): the scan's sensor
        frame into the map frame at the centre of the window), the uint16 pyramid of field_pyramid -> one CORR_DTYPE record: the node of
        smallest (sum_d2, index) over every rotation and every whole-cell offset of the window"""
        g = _field_cfg(field_cfg)
        p = _scan(points, 0, "the scan")
        st = _states(rot_states, np.float32, "the anchor states", CORR_MAX_ROT)
        k = _corr_cfg(corr_cfg, len(st))
        py = self._pyramid_planes(pyramid, g, k.levels)
        rec = np.zeros(1, CORR_DTYPE)
        self._ck(self._L.rr_correlate_scan(self._h, p.ctypes.data if len(p) else None, len(p), len(p), st.ctypes.data, len(st), py.ctypes.data,
                                           C.byref(g), C.byref(k), rec.ctypes.data))
        return rec[0]

    # ---- beam model (rr_cast.hip): a scan's first detection per azimuth, the map cast at pose hypotheses, a scan's rays scored against it
    def _beam_cfg(self, beam_cfg):
        """an RRBeamConfig or a dict of beam_config's arguments (n_cells is this context's), held to this context's n_cells"""
        n_cells, _ = self._polar_shape()
        if isinstance(beam_cfg, RRBeamConfig):
            if any(beam_cfg.reserved_):
                raise ValueError("reserved must be 0")
            return beam_config(beam_cfg.bin_begin, beam_cfg.bin_end, n_cells, beam_cfg.bin_step, beam_cfg.tol_bins, beam_cfg.clip_bins)
        if isinstance(beam_cfg, dict):
            return beam_config(n_cells=n_cells, **beam_cfg)
        raise ValueError("a beam config must be an RRBeamConfig (native.beam_config makes one) or a dict of its arguments, got %r" % (beam_cfg,))

    def _cast_inputs(self, states, n_max, dirs, field, g):
        """the host arrays of the two ray calls, checked -> (float32 states [n][4], float32 dirs [n_angles][2], the uint16 field)"""
        _, n_angles = self._polar_shape()
        st = _states(states, np.float32, "states", n_max)
        d = np.asarray(dirs)
        if d.dtype.kind not in "fiu" or d.shape != (n_angles, 2):
            raise ValueError("dirs must be real numbers of shape [%d][2] (beam_directions makes them), got %s %s" % (n_angles, d.dtype, d.shape))
        return st, np.ascontiguousarray(d, np.float32), self._field_grid(field, g, np.uint16, "field")

    def scan_profile_device(self, d_points_ptr, d_offsets_ptr, n_frames, max_points, d_first_bin_ptr, stream=None):
        """rr_scan_profile_device: uint16 [n_frames][n_angles] at d_first_bin_ptr, per azimuth INDEX the bin of the first detection among
        the points [n_frames][max_points] and offsets [n_frames][n_angles + 1] rr_detect_device wrote, n_cells where there is none"""
        n_cells, _ = self._polar_shape()
        _int_in(n_cells, 1, BEAM_MAX_CELLS, "n_cells")
        n, mp = _frames_arg(n_frames), _int_in(max_points, 0, ICP_MAX_POINTS, "max_points")
        if not d_offsets_ptr or not d_first_bin_ptr or (mp > 0 and not d_points_ptr):
            raise ValueError("scan_profile_device needs point, offset and profile buffers")
        self._ck(self._L.rr_scan_profile_device(self._h, d_points_ptr, d_offsets_ptr, n, mp, d_first_bin_ptr, stream))

    def scan_profile(self, points_list, offsets):
        """rr_scan_profile on what detect() returned: a list of n POINT_DTYPE arrays and offsets uint32 [n][n_angles + 1] -> uint16
        [n][n_angles]"""
        n_cells, n_angles = self._polar_shape()
        _int_in(n_cells, 1, BEAM_MAX_CELLS, "n_cells")
        buf, offs, _ = self._posed_clouds(points_list, offsets, None)
        out = np.zeros((len(buf), n_angles), np.uint16)
        self._ck(self._L.rr_scan_profile(self._h, buf.ctypes.data, offs.ctypes.data, len(buf), buf.shape[1], out.ctypes.data))
        return out

    def cast_map_device(self, d_states_ptr, n_hyp, d_dirs_ptr, d_field_ptr, field_cfg, beam_cfg, d_ranges_ptr, stream=None):
        """rr_cast_map_device: uint16 [n_hyp][n_angles] at d_ranges_ptr, the expected bin of every azimuth of the float32 states [n_hyp][4]
        = (c, s, tx, ty), each the sensor frame into the map frame, on the uint16 field of distance_field_device; d_dirs_ptr: float32
        [n_angles][2]; one launch on `stream`"""
        g, b, n = _cast_cfg(field_cfg), self._beam_cfg(beam_cfg), _int_in(n_hyp, 1, CAST_MAX_HYP, "n_hyp")
        if not d_states_ptr or not d_dirs_ptr or not d_field_ptr or not d_ranges_ptr:
            raise ValueError("cast_map_device needs state, direction, field and range buffers")
        self._ck(self._L.rr_cast_map_device(self._h, d_states_ptr, n, d_dirs_ptr, d_field_ptr, C.byref(g), C.byref(b), d_ranges_ptr, stream))

    def cast_map(self, states, dirs, field, field_cfg, beam_cfg):
        """rr_cast_map: float32 states [n][4], the table of beam_directions, the uint16 field of distance_field -> uint16 [n][n_angles]:
        the expected scan of the map at each pose, bin_end where a ray meets nothing"""
        g, b = _cast_cfg(field_cfg), self._beam_cfg(beam_cfg)
        st, d, f = self._cast_inputs(states, CAST_MAX_HYP, dirs, field, g)
        out = np.zeros((len(st), len(d)), np.uint16)
        self._ck(self._L.rr_cast_map(self._h, st.ctypes.data, len(st), d.ctypes.data, f.ctypes.data, C.byref(g), C.byref(b), out.ctypes.data))
        return out

    def score_beams_device(self, d_first_bin_ptr, d_states_ptr, n_hyp, d_dirs_ptr, d_field_ptr, field_cfg, beam_cfg, d_recs_ptr, stream=None):
        """rr_score_beams_device: BEAM_DTYPE records [n_hyp] in HBM for the float32 states [n_hyp][4] against ONE profile uint16 [n_angles]
        (a row of scan_profile_device); one launch on `stream`"""
        g, b, n = _cast_cfg(field_cfg), self._beam_cfg(beam_cfg), _int_in(n_hyp, 1, FIELD_MAX_HYP, "n_hyp")
        if not d_first_bin_ptr or not d_states_ptr or not d_dirs_ptr or not d_field_ptr or not d_recs_ptr:
            raise ValueError("score_beams_device needs profile, state, direction, field and record buffers")
        self._ck(self._L.rr_score_beams_device(self._h, d_first_bin_ptr, d_states_ptr, n, d_dirs_ptr, d_field_ptr, C.byref(g), C.byref(b), d_recs_ptr,
                                               stream))

    def score_beams(self, first_bin, states, dirs, field, field_cfg, beam_cfg):
        """rr_score_beams: one profile uint16 [n_angles] (a row of scan_profile), float32 states [n][4], the table of beam_directions, the
        uint16 field of distance_field -> BEAM_DTYPE [n]; more n_agree is better, n_through counts the rays that saw through a wall"""
        g, b = _cast_cfg(field_cfg), self._beam_cfg(beam_cfg)
        st, d, f = self._cast_inputs(states, FIELD_MAX_HYP, dirs, field, g)
        fb = np.asarray(first_bin)
        if fb.dtype != np.uint16 or fb.shape != (len(d),):
            raise ValueError("the profile must be uint16 [%d], got %s %s" % (len(d), fb.dtype, fb.shape))
        fb = np.ascontiguousarray(fb)
        recs = np.zeros(len(st), BEAM_DTYPE)
        self._ck(self._L.rr_score_beams(self._h, fb.ctypes.data, st.ctypes.data, len(st), d.ctypes.data, f.ctypes.data, C.byref(g), C.byref(b),
                                        recs.ctypes.data))
        return recs

    # ---- object annotations (rr_notes.hip): one record per object from label images; any context with a config, mesh or not
    def _label_planes(self, planes, what="label planes"):
        """uint32 [n][n_cells][n_angles] (or one plane) of this context's shape -> contiguous 3-D array"""
        n_cells, n_angles = self._polar_shape()
        x = np.asarray(planes)
        if x.dtype != np.uint32:
            raise ValueError("%s must be uint32, got dtype %s" % (what, x.dtype))
        if x.ndim == 2:
            x = x[None]
        if x.ndim != 3 or x.shape[1:] != (n_cells, n_angles) or not 1 <= x.shape[0] <= 65535:
            raise ValueError("%s must have shape [n][%d][%d] (n in 1..65535), got %s" % (what, n_cells, n_angles, np.asarray(planes).shape))
        return np.ascontiguousarray(x)

    def annotate_scratch_bytes(self, n_frames, n_objects):
        """rr_annotate_scratch_bytes for this context's n_angles"""
        self._polar_shape()
        return int(self._L.rr_annotate_scratch_bytes(_frames_arg(n_frames), _int_in(n_objects, 1, 0xFFFFFE, "n_objects"), int(self.n_angles)))

    def annotate_labels_device(self, d_labels_ptr, d_imgs_ptr, n_frames, n_objects, d_notes_ptr, d_skipped_ptr, d_scratch_ptr, scratch_bytes,
                               extent=NOTE_DIRECT, stream=None):
        """rr_annotate_labels_device: NOTE_DTYPE records [n_frames][n_objects] and skip counts uint32 [n_frames] in HBM, on `stream`;
        d_imgs_ptr None: peak and sum are 0.  The scratch (annotate_scratch_bytes, 16-byte aligned) is the caller's."""
        self._polar_shape()
        n, k, m = _frames_arg(n_frames), _int_in(n_objects, 1, 0xFFFFFE, "n_objects"), note_mask(extent)
        if not d_labels_ptr or not d_notes_ptr or not d_skipped_ptr or not d_scratch_ptr:
            raise ValueError("annotate_labels_device needs label, record, skip-count and scratch buffers")
        self._ck(self._L.rr_annotate_labels_device(self._h, d_labels_ptr, d_imgs_ptr, n, k, m, d_notes_ptr, d_skipped_ptr, d_scratch_ptr,
                                                   int(scratch_bytes), stream))

    def annotate_labels(self, labels, imgs=None, n_objects=None, extent=NOTE_DIRECT):
        """rr_annotate_labels on host planes [n][n_cells][n_angles] (or one plane) -> (NOTE_DTYPE [n][n_objects], skipped uint32 [n]).
        n_objects None: the mesh's object count."""
        x = self._label_planes(labels)
        z = None if imgs is None else self._polar_images(imgs)
        if z is not None and z.shape != x.shape:
            raise ValueError("%d label planes with %d images" % (len(x), len(z)))
        k = _int_in(self.n_objects if n_objects is None else n_objects, 1, 0xFFFFFE, "n_objects")
        notes = np.zeros((len(x), k), NOTE_DTYPE)
        skipped = np.zeros(len(x), np.uint32)
        self._ck(self._L.rr_annotate_labels(self._h, x.ctypes.data, _ptr(z), len(x), k, note_mask(extent),
                                            notes.ctypes.data, skipped.ctypes.data))
        return notes, skipped

    def label_points_device(self, d_points_ptr, d_offsets_ptr, n_frames, max_points, d_labels_ptr, d_point_labels_ptr, d_faces_ptr=None,
                            d_point_faces_ptr=None, d_vel_img_ptr=None, d_point_vel_ptr=None, stream=None):
        """rr_label_points_device: for the points rr_detect_device wrote, the label (and face, range rate) under each, uint32 / float32
        [n_frames][max_points] in HBM, on `stream`"""
        self._polar_shape()
        n, mp = _frames_arg(n_frames), _int_in(max_points, 0, 2**31 - 1, "max_points")
        if not d_points_ptr or not d_offsets_ptr or not d_labels_ptr or not d_point_labels_ptr:
            raise ValueError("label_points_device needs point, offset, label and output buffers")
        if bool(d_faces_ptr) != bool(d_point_faces_ptr) or bool(d_vel_img_ptr) != bool(d_point_vel_ptr):
            raise ValueError("a source plane and its per-point output come together")
        self._ck(self._L.rr_label_points_device(self._h, d_points_ptr, d_offsets_ptr, n, mp, d_labels_ptr, d_faces_ptr, d_vel_img_ptr,
                                                d_point_labels_ptr, d_point_faces_ptr, d_point_vel_ptr, stream))

    def polar_to_cartesian_labels_device(self, d_planes_ptr, n_frames, width, pixel_size, d_out_ptr, stream=None):
        """rr_polar_to_cartesian_labels_device: uint32 [n_frames][width][width] in HBM by the nearest rule, on `stream`"""
        self._polar_shape()
        c = cartesian_config(width, pixel_size, False)
        n = _frames_arg(n_frames)
        if not d_planes_ptr or not d_out_ptr:
            raise ValueError("polar_to_cartesian_labels_device needs plane and output buffers")
        self._ck(self._L.rr_polar_to_cartesian_labels_device(self._h, d_planes_ptr, n, C.byref(c), d_out_ptr, stream))

    def polar_to_cartesian_labels(self, planes, width, pixel_size):
        """rr_polar_to_cartesian_labels on host planes [n][n_cells][n_angles] (or one plane) -> uint32 [n][width][width]"""
        x = self._label_planes(planes, "planes")
        c = cartesian_config(width, pixel_size, False)
        out = np.zeros((len(x), c.width, c.width), np.uint32)
        self._ck(self._L.rr_polar_to_cartesian_labels(self._h, x.ctypes.data, len(x), C.byref(c), out.ctypes.data))
        return out

    def simulate_batch_annotations(self, poses, extent=NOTE_DIRECT, want_images=False):
        """rr_simulate_batch_annotations: poses [n][7] -> (NOTE_DTYPE [n][n_objects], skipped uint32 [n], images uint8 [n][n_cells][n_angles]
        or None); no label plane leaves the GPU"""
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 7)
        n_cells, n_angles = self._polar_shape()
        notes = np.zeros((len(p), self.n_objects), NOTE_DTYPE)
        skipped = np.zeros(len(p), np.uint32)
        imgs = np.zeros((len(p), n_cells, n_angles), np.uint8) if want_images else None
        self._ck(self._L.rr_simulate_batch_annotations(self._h, p.ctypes.data, len(p), note_mask(extent), _ptr(imgs),
                                                       notes.ctypes.data, skipped.ctypes.data))
        return notes, skipped, imgs

    def synchronize(self, stream=None):
        self._ck(self._L.rr_synchronize(self._h, stream))

    def stats(self):
        st = RRStats()
        self._ck(self._L.rr_get_stats(self._h, C.byref(st)))
        return st.asdict()

    def set_stats_mode(self, on):
        self._ck(self._L.rr_set_stats_mode(self._h, int(bool(on))))

    def set_timing_mode(self, on):
        self._ck(self._L.rr_set_timing_mode(self._h, int(on)))

    def kernel_time(self, name, reset=False):
        ms, n = C.c_double(), C.c_uint64()
        self._ck(self._L.rr_get_kernel_time(self._h, name.encode(), C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    def kernel_samples(self, name):
        """Every launch duration (ms) recorded for `name` since the last reset."""
        n = C.c_size_t()
        self._ck(self._L.rr_get_kernel_samples(self._h, name.encode(), None, 0, C.byref(n)))
        out = np.zeros(n.value, np.float32)
        if n.value:
            self._ck(self._L.rr_get_kernel_samples(self._h, name.encode(), out.ctypes.data, n.value, C.byref(n)))
        return out

    def reserve_timing_events(self, n):
        self._ck(self._L.rr_reserve_timing_events(self._h, int(n)))

    def trace_grid(self):
        """rr_get_trace_grid -> (rows[24] of the last call, hist[24], repaired 16-ray groups)"""
        rows = np.zeros(24, np.uint32); hist = np.zeros(24, np.uint32); rep = C.c_uint64()
        self._ck(self._L.rr_get_trace_grid(self._h, rows.ctypes.data, hist.ctypes.data, C.byref(rep)))
        return rows, hist, int(rep.value)

    def graph_stats(self):
        """rr_get_graph_stats -> (launch chains captured, replayed)"""
        a, b = C.c_uint64(), C.c_uint64()
        self._ck(self._L.rr_get_graph_stats(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def bvh_info(self):
        a, b, d, s = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint32()
        self._ck(self._L.rr_get_bvh_info(self._h, C.byref(a), C.byref(b), C.byref(d), C.byref(s)))
        return {"n_nodes": a.value, "n_tris": b.value, "depth": d.value, "stack_need": s.value}

    def debug_trace(self, origs, dirs):
        o = np.ascontiguousarray(origs, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        t = np.zeros(len(o), np.float32)
        f = np.zeros(len(o), np.uint32)
        self._ck(self._L.rr_debug_trace(self._h, o.ctypes.data, d.ctypes.data, len(o), t.ctypes.data, f.ctypes.data))
        return t, f

    def debug_fresnel(self, normals, dirs, energy, v1, v2):
        """rr_debug_fresnel: the kernels' fresnel_split on n inputs -> (refl_dir [n][3] f32, refl_energy [n] f64, refr_dir, refr_energy)"""
        nr = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = len(d)
        e = np.ascontiguousarray(np.broadcast_to(np.asarray(energy, np.float64), (n,)))
        a = np.ascontiguousarray(np.broadcast_to(np.asarray(v1, np.float64), (n,)))
        b = np.ascontiguousarray(np.broadcast_to(np.asarray(v2, np.float32), (n,)))
        rd, td = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        re, te = np.zeros(n, np.float64), np.zeros(n, np.float64)
        self._ck(self._L.rr_debug_fresnel(self._h, n, nr.ctypes.data, d.ctypes.data, e.ctypes.data, a.ctypes.data, b.ctypes.data,
                                          rd.ctypes.data, re.ctypes.data, td.ctypes.data, te.ctypes.data))
        return rd, re, td, te

    def debug_brdf(self, angle, energy, ambient, diffuse, specular, brdf_model=0):
        """rr_debug_brdf: the kernels' back_reflection_shader on n inputs (arrays or scalars, broadcast) -> [n] f32"""
        cols = np.broadcast_arrays(*[np.asarray(x, np.float32) for x in (angle, energy, ambient, diffuse, specular)])
        x = np.ascontiguousarray(np.stack([c.reshape(-1) for c in cols], 1), np.float32)
        out = np.zeros(len(x), np.float32)
        self._ck(self._L.rr_debug_brdf(self._h, len(x), x.ctypes.data, int(brdf_model), out.ctypes.data))
        return out

    def debug_column(self, n_frames, n_loc, az_begin=0, n_passes=1, n_beam=0, record_multi_path=False,
                     echoes=None, echo_count=None, slots=None, slot_hit=None, slot_count=None):
        """rr_debug_column: k_column on caller-given echo streams of n_seg = n_frames * n_loc segments, under the context's
        config and noise offsets.  echoes [n_seg][list_stride] / echo_count [n_seg]: the compacted list (ECHO_DTYPE records);
        slots [n_seg][2 * slot_stride] / slot_hit [n_seg][slot_stride] / slot_count [n_seg]: the last pass' per-wave slots.
        Returns (f32 [n_seg][n_cells], u8 [n_seg][n_cells], stats [n_seg][3] = wave_passes, hits, signals of the last pass)."""
        n_seg = int(n_frames) * int(n_loc)
        n_cells = self.cfg.n_cells if self.cfg is not None else 1   # unconfigured: the library reports it
        ls = ss = 0
        e = ec = sl = sh = sc = None
        if echoes is not None:
            e = np.ascontiguousarray(echoes, ECHO_DTYPE).reshape(n_seg, -1)
            ec = np.ascontiguousarray(echo_count, np.uint32).reshape(n_seg)
            ls = e.shape[1]
        if slots is not None:
            sl = np.ascontiguousarray(slots, ECHO_DTYPE).reshape(n_seg, -1)
            if sl.shape[1] % 2:
                raise ValueError("slots must hold an even and an odd record per wave")
            ss = sl.shape[1] // 2
            sh = np.ascontiguousarray(slot_hit, np.uint8).reshape(n_seg, ss)
            if slot_count is not None:
                sc = np.ascontiguousarray(slot_count, np.uint32).reshape(n_seg)
        f32 = np.zeros((max(n_seg, 0), n_cells), np.float32)
        u8 = np.zeros((max(n_seg, 0), n_cells), np.uint8)
        st = np.zeros((max(n_seg, 0), 3), np.uint32)
        self._ck(self._L.rr_debug_column(self._h, int(n_frames), int(n_loc), int(az_begin), int(n_passes), int(n_beam),
                                         int(bool(record_multi_path)), _ptr(e), _ptr(ec), ls, _ptr(sl), _ptr(sh), _ptr(sc), ss,
                                         f32.ctypes.data, u8.ctypes.data, st.ctypes.data))
        return f32, u8, st

    # ---- echo provenance (include/radarays_mi355.h): per-echo face / object / pass / kind, label images
    def simulate_batch_provenance_device(self, poses, d_imgs_ptr, d_labels_ptr=None, d_faces_ptr=None, d_echoes_ptr=None, echo_stride=0,
                                         d_echo_counts_ptr=None, stream=None):
        """rr_simulate_batch_provenance_device: the images of rr_simulate_batch_device and, in HBM, any of: label / face planes uint32
        [n][n_cells][n_angles], the echo stream ECHO_SRC_DTYPE [n][n_angles][echo_stride] with its true counts uint32 [n][n_angles]."""
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 7)
        self._ck(self._L.rr_simulate_batch_provenance_device(self._h, p.ctypes.data, len(p), d_imgs_ptr, d_labels_ptr, d_faces_ptr, d_echoes_ptr,
                                                             int(echo_stride), d_echo_counts_ptr, stream))

    def simulate_provenance(self, pose, echo_stride=None, want_labels=True, want_faces=True):
        """rr_simulate_provenance: one frame -> (u8 [n_cells][n_angles], labels uint32 or None, faces uint32 or None, echoes ECHO_SRC_DTYPE
        [n_angles][echo_stride], counts uint32 [n_angles]).  echo_stride None: every echo (a first call for the counts sizes the rows);
        0: no echo stream (echoes None, counts still true)."""
        p = np.ascontiguousarray(pose, np.float32)
        if p.shape != (7,):
            raise ValueError("pose must be [7] (qx qy qz qw tx ty tz), got %s" % (p.shape,))
        n_cells = self.cfg.n_cells if self.cfg is not None else 1   # unconfigured: the library reports it
        A = self.n_angles
        u8 = np.zeros((n_cells, A), np.uint8)
        lab = np.full((n_cells, A), LABEL_NONE, np.uint32) if want_labels else None
        fac = np.full((n_cells, A), LABEL_NONE, np.uint32) if want_faces else None
        cnt = np.zeros(A, np.uint32)
        if echo_stride is None:
            self._ck(self._L.rr_simulate_provenance(self._h, p.ctypes.data, u8.ctypes.data, None, None, None, 0, cnt.ctypes.data))
            echo_stride = max(int(cnt.max()), 1)
        echo_stride = _int_in(echo_stride, 0, 1 << 30, "echo_stride")
        ech = np.zeros((A, echo_stride), ECHO_SRC_DTYPE) if echo_stride else None
        self._ck(self._L.rr_simulate_provenance(self._h, p.ctypes.data, u8.ctypes.data, _ptr(lab), _ptr(fac), _ptr(ech), echo_stride, cnt.ctypes.data))
        return u8, lab, fac, ech, cnt

    # ---- wave paths (include/radarays_mi355.h): every ray-cast wave's ray, hit, parent and echo per azimuth
    def simulate_batch_paths_device(self, poses, d_imgs_ptr, d_waves_ptr=None, wave_stride=0, d_wave_counts_ptr=None, d_pass_counts_ptr=None,
                                    flags=0, stream=None):
        """rr_simulate_batch_paths_device: the images of rr_simulate_batch_device and, in HBM, the wave lists WAVE_DTYPE
        [n][n_angles][wave_stride] with their true counts uint32 [n][n_angles] and the waves per pass uint32 [n][n_angles][16]."""
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 7)
        self._ck(self._L.rr_simulate_batch_paths_device(self._h, p.ctypes.data, len(p), d_imgs_ptr, d_waves_ptr, int(wave_stride),
                                                        d_wave_counts_ptr, d_pass_counts_ptr, int(flags), stream))

    def simulate_paths(self, pose, wave_stride=None, map_frame=False):
        """rr_simulate_paths: one frame -> (u8 [n_cells][n_angles], waves WAVE_DTYPE [n_angles][wave_stride], counts uint32 [n_angles],
        pass_counts uint32 [n_angles][16]).  wave_stride None: every wave (a first call for the counts sizes the rows); 0: no records
        (waves None, counts still true)."""
        p = np.ascontiguousarray(pose, np.float32)
        if p.shape != (7,):
            raise ValueError("pose must be [7] (qx qy qz qw tx ty tz), got %s" % (p.shape,))
        n_cells = self.cfg.n_cells if self.cfg is not None else 1   # unconfigured: the library reports it
        A = self.n_angles
        u8 = np.zeros((n_cells, A), np.uint8)
        cnt = np.zeros(A, np.uint32)
        pc = np.zeros((A, WAVES_MAX_PASSES), np.uint32)
        flags = WAVES_MAP_FRAME if map_frame else 0
        if wave_stride is None:
            self._ck(self._L.rr_simulate_paths(self._h, p.ctypes.data, u8.ctypes.data, None, 0, cnt.ctypes.data, None, flags))
            wave_stride = max(int(cnt.max()), 1)
        wave_stride = _int_in(wave_stride, 0, 1 << 26, "wave_stride")
        wav = np.zeros((A, wave_stride), WAVE_DTYPE) if wave_stride else None
        self._ck(self._L.rr_simulate_paths(self._h, p.ctypes.data, u8.ctypes.data, _ptr(wav), wave_stride,
                                           cnt.ctypes.data, pc.ctypes.data, flags))
        return u8, wav, cnt, pc

    # ---- Doppler (include/radarays_mi355.h): per-echo range rate and the FMCW range shift it causes
    def simulate_batch_doppler_device(self, poses, gain, d_imgs_ptr, sensor_vel=None, d_echo_vel_ptr=None, echo_stride=0, d_echo_counts_ptr=None,
                                      d_echo_cells_ptr=None, d_vel_img_ptr=None, stream=None):
        """rr_simulate_batch_doppler_device: the images of the shifted echo stream and, in HBM, any of: v_r float32 / cell' int32
        [n][n_angles][echo_stride] with their true counts uint32 [n][n_angles], the winner's v_r float32 [n][n_cells][n_angles].
        sensor_vel [n][3] (map frame, m/s) or None: 0; gain: kappa in seconds."""
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 7)
        v = None if sensor_vel is None else np.ascontiguousarray(sensor_vel, np.float32).reshape(-1, 3)
        if v is not None and len(v) != len(p):
            raise ValueError("sensor_vel must hold one velocity per pose: %d poses, %d velocities" % (len(p), len(v)))
        self._ck(self._L.rr_simulate_batch_doppler_device(self._h, p.ctypes.data, len(p), _ptr(v), float(gain), d_imgs_ptr,
                                                          d_echo_vel_ptr, int(echo_stride), d_echo_counts_ptr, d_echo_cells_ptr, d_vel_img_ptr, stream))

    def simulate_doppler(self, pose, sensor_vel=None, gain=0.0, echo_stride=None, want_f32=False, want_vel_img=True):
        """rr_simulate_doppler: one frame -> (u8 [n_cells][n_angles], f32 image or None, v_r float32 [n_angles][echo_stride], cell' int32
        [n_angles][echo_stride], counts uint32 [n_angles], velocity image float32 [n_cells][n_angles] or None).  echo_stride None: every
        echo (a first call for the counts sizes the rows); 0: no rows (None, counts still true)."""
        p = np.ascontiguousarray(pose, np.float32)
        if p.shape != (7,):
            raise ValueError("pose must be [7] (qx qy qz qw tx ty tz), got %s" % (p.shape,))
        v = None if sensor_vel is None else np.ascontiguousarray(sensor_vel, np.float32)
        if v is not None and v.shape != (3,):
            raise ValueError("sensor_vel must be [3] (vx vy vz), got %s" % (v.shape,))
        n_cells = self.cfg.n_cells if self.cfg is not None else 1   # unconfigured: the library reports it
        A = self.n_angles
        u8 = np.zeros((n_cells, A), np.uint8)
        f32 = np.zeros((n_cells, A), np.float32) if want_f32 else None
        img = np.full((n_cells, A), np.nan, np.float32) if want_vel_img else None
        cnt = np.zeros(A, np.uint32)
        if echo_stride is None:
            self._ck(self._L.rr_simulate_doppler(self._h, p.ctypes.data, _ptr(v), float(gain), u8.ctypes.data, None, None, 0, cnt.ctypes.data, None, None))
            echo_stride = max(int(cnt.max()), 1)
        echo_stride = _int_in(echo_stride, 0, 1 << 26, "echo_stride")
        vel = np.zeros((A, echo_stride), np.float32) if echo_stride else None
        cel = np.full((A, echo_stride), -1, np.int32) if echo_stride else None
        self._ck(self._L.rr_simulate_doppler(self._h, p.ctypes.data, _ptr(v), float(gain), u8.ctypes.data, _ptr(f32), _ptr(vel), echo_stride, cnt.ctypes.data,
                                             _ptr(cel), _ptr(img)))
        return u8, f32, vel, cel, cnt, img

    def debug_labels(self, echoes, counts, az_begin=0):
        """rr_debug_labels: the label kernel on caller-given streams, echoes ECHO_SRC_DTYPE [n_seg][stride], counts [n_seg], under the
        context's config (denoiser, n_cells) -> (labels, faces), each uint32 [n_seg][n_cells], not assembled."""
        cnt = np.ascontiguousarray(counts, np.uint32).ravel()
        n_seg = len(cnt)
        e = np.ascontiguousarray(echoes, ECHO_SRC_DTYPE).reshape(max(n_seg, 1), -1)
        n_cells = self.cfg.n_cells if self.cfg is not None else 1
        lab = np.zeros((n_seg, n_cells), np.uint32)
        fac = np.zeros((n_seg, n_cells), np.uint32)
        self._ck(self._L.rr_debug_labels(self._h, n_seg, int(az_begin), e.ctypes.data if e.size else None, cnt.ctypes.data, e.shape[1],
                                         lab.ctypes.data, fac.ctypes.data))
        return lab, fac


class HostImages:
    """Page-locked host memory for images (rr_host_alloc), viewed as a numpy array."""

    def __init__(self, shape):
        self._L = lib()
        self.shape = tuple(int(x) for x in shape)
        n = int(np.prod(self.shape))
        self.ptr = self._L.rr_host_alloc(n)
        if not self.ptr:
            raise RRError("rr_host_alloc(%d) failed" % n)
        self.array = np.ctypeslib.as_array((C.c_uint8 * n).from_address(self.ptr)).reshape(self.shape)

    def close(self):
        if getattr(self, "ptr", None):
            self.array = None
            self._L.rr_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cone_dirs(width_rad, sample_dist, p_in_cone, u_angle, r_variate):
    """rr_cone_dirs (host only): sample_cone_local's geometry on given variates -> [n][3] float32."""
    u = np.ascontiguousarray(u_angle, np.float32); r = np.ascontiguousarray(r_variate, np.float32)
    out = np.zeros((len(u), 3), np.float32)
    rc = lib().rr_cone_dirs(float(width_rad), int(sample_dist), float(p_in_cone), u.ctypes.data, r.ctypes.data, len(u), out.ctypes.data)
    if rc:
        raise RRError("rr_cone_dirs: rc=%d" % rc)
    return out


def sample_cone_local(seed, width_rad, n, sample_dist=2, p_in_cone=0.8):
    """rr_sample_cone_local (host only): the C twin of beams.sample_cone_local."""
    out = np.zeros((int(n), 3), np.float32)
    rc = lib().rr_sample_cone_local(int(seed), float(width_rad), int(n), int(sample_dist), float(p_in_cone), out.ctypes.data)
    if rc:
        raise RRError("rr_sample_cone_local: rc=%d" % rc)
    return out


def load_mesh_file(path, object_order=None):
    """rr_load_mesh_file (host only): PLY / OBJ / DAE -> {"verts", "faces", "face_object_id", "n_objects", "object_names"}.
    object_order: names in the order their ids should run (rr_mesh_reorder_objects: the file's own numbering is depth-first
    scene order -- a material list written for another numbering, e.g. rmagine's, is matched by naming the objects)."""
    m = RRMesh()
    err = C.create_string_buffer(512)
    rc = lib().rr_load_mesh_file(str(path).encode(), C.byref(m), err, len(err))
    if rc:
        raise RRError("%s (rc=%d)" % (err.value.decode(errors="replace"), rc))
    try:
        if object_order:
            names = (C.c_char_p * len(object_order))(*[str(x).encode() for x in object_order])
            rc = lib().rr_mesh_reorder_objects(C.byref(m), names, len(object_order), err, len(err))
            if rc:
                raise RRError("%s (rc=%d)" % (err.value.decode(errors="replace"), rc))
        out = {"verts": np.ctypeslib.as_array(m.verts, (m.n_verts, 3)).copy() if m.n_verts else np.zeros((0, 3), np.float32),
               "faces": np.ctypeslib.as_array(m.faces, (m.n_faces, 3)).copy() if m.n_faces else np.zeros((0, 3), np.uint32),
               "face_object_id": np.ctypeslib.as_array(m.face_object_id, (m.n_faces,)).copy() if m.n_faces else np.zeros(0, np.uint32),
               "n_objects": int(m.n_objects),
               "object_names": [m.object_names[k].decode(errors="replace") for k in range(m.n_objects)] if m.object_names else []}
    finally:
        lib().rr_free_mesh(C.byref(m))
    return out


def partition(n_angles, world, rank):
    """rr_partition: the azimuth block [begin, end) of `rank` (pure host arithmetic, no GPU needed)."""
    b, e = C.c_int(), C.c_int()
    lib().rr_partition(int(n_angles), int(world), int(rank), C.byref(b), C.byref(e))
    return b.value, e.value


def multi_plan(n_angles, n_cells, n_devices, n_frames):
    """rr_multi_plan -> (equal, bytes_per_device, send_off[r][f], recv_off[r][f], piece_bytes[r][f])"""
    eq, bpd = C.c_int(), C.c_size_t()
    so = np.zeros((n_devices, n_frames), np.uint64); ro = np.zeros_like(so); pb = np.zeros_like(so)
    assert C.sizeof(C.c_size_t) == 8
    rc = lib().rr_multi_plan(n_angles, n_cells, n_devices, n_frames, C.byref(eq), C.byref(bpd), so.ctypes.data, ro.ctypes.data, pb.ctypes.data)
    if rc:
        raise RRError("rr_multi_plan: rc=%d" % rc)
    return bool(eq.value), int(bpd.value), so, ro, pb


class MultiContext(_Scene):
    """rr_multi: several GPUs of one node behind one object (one process; RCCL inside the library).  The scene setters reach every device."""
    _PREFIX = "rr_multi_"

    def __init__(self, devices):
        self._L = lib()
        d = (C.c_int * len(devices))(*[int(x) for x in devices])
        self._h = self._L.rr_create_multi(d, len(devices))
        if not self._h:
            raise RRError(self._L.rr_multi_last_error(None).decode())
        self.cfg = None
        self.n_angles = 400
        self.n_objects = 1

    def close(self):
        if getattr(self, "_h", None):
            self._L.rr_destroy_multi(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rccl_version(self):
        """NCCL version code of the RCCL library behind the communicator (0: none)"""
        return int(self._L.rr_multi_rccl_version(self._h))

    def device_count(self):
        return self._L.rr_multi_device_count(self._h)

    def tree_cost(self):
        """device 0's (cost now, cost as built): every device holds the same tree"""
        a, b = C.c_double(), C.c_double()
        h = self._L.rr_multi_ctx(self._h, 0)
        rc = self._L.rr_get_tree_cost(h, C.byref(a), C.byref(b))
        if rc != 0:
            raise RRError("%s (rc=%d)" % (self._L.rr_last_error(h).decode(), rc))
        return a.value, b.value

    def simulate_batch(self, poses):
        """-> uint8 [n][n_cells][n_angles] in host memory."""
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 7)
        out = np.zeros((len(p), self.cfg.n_cells, self.n_angles), np.uint8)
        self._ck(self._L.rr_multi_simulate_batch(self._h, p.ctypes.data, len(p), out.ctypes.data))
        return out

    def simulate(self, pose):
        return self.simulate_batch([pose])[0]

    def simulate_batch_async(self, poses, h_imgs_ptr):
        """Pipelined: enqueue the batch, images [n][n_cells][n_angles] arrive at h_imgs_ptr (page-locked: HostImages);
        complete after wait(h_imgs_ptr)."""
        p = np.ascontiguousarray(poses, np.float32).reshape(-1, 7)
        self._ck(self._L.rr_multi_simulate_batch_async(self._h, p.ctypes.data, len(p), h_imgs_ptr))

    def wait(self, h_imgs_ptr=None):
        self._ck(self._L.rr_multi_wait(self._h, h_imgs_ptr))
