"""Occupancy mapping of include/radarays_mi355.h (rr_occupancy_update, rr_occupancy_map) restated in numpy: f32 where the definition says f32
(numpy rounds every operation and fuses none), integers everywhere else.  The point mapping and the cell rule are field_ref's, the polar
geometry is that of detect_ref.cartesian (rr_polar.h).  The GPU tests compare the profile, the hits and the map against it bit for bit, and
the free pass up to the cells that the device's atan2f puts on the other side of an azimuth border; the host tests hold the profile and
the hit step to a brute-force f64 version."""
import collections
import math

import numpy as np

import field_ref as F
from radarays_ros_amd import native

f32 = np.float32

# the polar geometry the update reads from the context's config
Polar = collections.namedtuple("Polar", "n_cells n_angles scroll theta_min theta_inc resolution")


def polar(n_cells, n_angles, scroll=0, theta_min=0.0, theta_inc=None, resolution=0.0438):
    """theta_inc None: the reference's clockwise sweep, as native.make_config"""
    inc = -(2.0 * np.pi) / n_angles if theta_inc is None else theta_inc
    return Polar(int(n_cells), int(n_angles), int(scroll) % int(n_angles), float(f32(theta_min)), float(f32(inc)), float(resolution))


def polar_of(rrcfg):
    """the geometry of an rr_config (native.make_config, Context._rrcfg)"""
    return polar(rrcfg.n_cells, rrcfg.n_angles, rrcfg.scroll_image, rrcfg.theta_min, rrcfg.theta_inc, rrcfg.resolution)


def model(l_hit=4, l_free=1, margin_bins=0, max_free_bin=0):
    return dict(l_hit=l_hit, l_free=l_free, margin_bins=margin_bins, max_free_bin=max_free_bin)


# ---- step 1 -----------------------------------------------------------------------------------------------------------------------------
def profile(clouds, offsets, G, m, max_points=None):
    """clouds: n POINT_DTYPE arrays, whole (a cloud longer than max_points loses its tail here); offsets uint32 [n][n_angles + 1] ->
    free2 float32 [n][n_angles], indexed by azimuth a = col - scroll (mod n_angles)"""
    offs = np.asarray(offsets, np.uint32).reshape(len(clouds), G.n_angles + 1).astype(np.int64)
    out = np.zeros((len(clouds), G.n_angles), np.float32)
    for f, cloud in enumerate(clouds):
        mp = len(cloud) if max_points is None else max_points
        bins = np.asarray(cloud)["bin"].astype(np.int64)
        for col in range(G.n_angles):
            first, nxt = offs[f, col], offs[f, col + 1]
            if nxt > first and first >= mp:
                free_bins = 0                                         # every detection of the column was cut: nothing is asserted
            else:
                fb = int(bins[first]) if nxt > first else G.n_cells
                free_bins = min(max(fb - m["margin_bins"], 0), m["max_free_bin"])
            r = f32(float(free_bins) * G.resolution)
            out[f, (col - G.scroll) % G.n_angles] = r * r
    return out


def profile_brute(clouds, G, m, max_points=None):
    """the same from the points alone, in f64 and without the offsets: per column the smallest bin among the points that survive max_points"""
    out = np.zeros((len(clouds), G.n_angles), np.float64)
    for f, cloud in enumerate(clouds):
        c = np.asarray(cloud)
        kept = c if max_points is None else c[:max_points]
        for col in range(G.n_angles):
            any_at_all = bool(np.any(c["column"] == col))
            mine = kept["bin"][kept["column"] == col].astype(np.int64)
            if any_at_all and len(mine) == 0:
                free_bins = 0
            else:
                fb = int(mine.min()) if len(mine) else G.n_cells
                free_bins = min(max(fb - m["margin_bins"], 0), m["max_free_bin"])
            out[f, (col - G.scroll) % G.n_angles] = (free_bins * G.resolution) ** 2
    return out


# ---- step 2 -----------------------------------------------------------------------------------------------------------------------------
def cell_centres(cfg):
    """(qx, qy) float32 [height][width]"""
    ix, iy = np.arange(cfg.width, dtype=np.float32), np.arange(cfg.height, dtype=np.float32)
    qx = f32(cfg.x0) + (ix + f32(0.5)) * f32(cfg.cell)
    qy = f32(cfg.y0) + (iy + f32(0.5)) * f32(cfg.cell)
    return np.broadcast_to(qx[None, :], (cfg.height, cfg.width)), np.broadcast_to(qy[:, None], (cfg.height, cfg.width))


def az_coord(phi, G):
    """rr_polar.h: the azimuth coordinate of a yaw, always in [0, n_angles)"""
    na = f32(G.n_angles)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        u = np.fmod((phi - f32(G.theta_min)) / f32(G.theta_inc), na).astype(np.float32)
        u = np.where(u < 0, u + na, u).astype(np.float32)
        u = np.where(u >= na, u - na, u).astype(np.float32)
        u = np.where((u >= 0) & (u < na), u, f32(0)).astype(np.float32)
    return u


def az_nearest(u, G):
    a = np.rint(u).astype(np.int64)
    return np.where(a >= G.n_angles, a - G.n_angles, a)


def sensor_frame(cfg, state):
    """the cell centres in the sensor frame of a state (c, s, tx, ty): (px, py, rho2, a)"""
    qx, qy = cell_centres(cfg)
    cf, sf, txf, tyf = (f32(v) for v in state)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = qx - txf, qy - tyf
        px = cf * dx + sf * dy
        py = cf * dy - sf * dx
        rho2 = px * px + py * py
        phi = np.arctan2(py, px).astype(np.float32)
    return px, py, rho2, phi


def free_counts(free2, cfg, G, states=None, az_shift=0):
    """-> (int64 [height][width]: in how many scans each cell is free, the azimuth index of every cell under the LAST scan).  az_shift: every
    cell reads the profile one azimuth to the side (the tests' allowance for the last place of atan2f)"""
    n = len(free2)
    count = np.zeros((cfg.height, cfg.width), np.int64)
    a = None
    for f in range(n):
        state = (1.0, 0.0, 0.0, 0.0) if states is None else tuple(np.asarray(states, np.float64)[f])
        _, _, rho2, phi = sensor_frame(cfg, state)
        a = az_nearest(az_coord(phi, G), G)
        with np.errstate(invalid="ignore"):
            count += rho2 < free2[f][(a + az_shift) % G.n_angles]
    return count, a


# ---- step 3 -----------------------------------------------------------------------------------------------------------------------------
def hit_counts(clouds, cfg, states=None, max_points=None):
    """int64 [height][width]: how many points fell into each cell"""
    count = np.zeros(cfg.height * cfg.width, np.int64)
    for f, cloud in enumerate(clouds):
        x, y = F.xy_of(cloud)
        if max_points is not None:
            x, y = x[:max_points], y[:max_points]
        state = (1.0, 0.0, 0.0, 0.0) if states is None else tuple(np.asarray(states, np.float64)[f])
        inside, index = F.cells(*F.move(x, y, state), cfg)
        np.add.at(count, index[inside], 1)
    return count.reshape(cfg.height, cfg.width)


def hit_counts_brute(clouds, cfg, states=None, max_points=None):
    """the same in f64 with a plain loop over the points (for inputs whose points sit away from cell edges)"""
    count = np.zeros((cfg.height, cfg.width), np.int64)
    for f, cloud in enumerate(clouds):
        c, s, tx, ty = (1.0, 0.0, 0.0, 0.0) if states is None else (float(v) for v in np.asarray(states, np.float64)[f])
        pts = np.asarray(cloud) if max_points is None else np.asarray(cloud)[:max_points]
        for p in pts:
            x, y = float(p["x"]), float(p["y"])
            u = ((c * x - s * y) + tx - float(f32(cfg.x0))) / float(f32(cfg.cell))
            v = ((s * x + c * y) + ty - float(f32(cfg.y0))) / float(f32(cfg.cell))
            if math.isfinite(u) and math.isfinite(v) and 0 <= u < cfg.width and 0 <= v < cfg.height:
                count[int(math.floor(v)), int(math.floor(u))] += 1
    return count


# ---- the calls --------------------------------------------------------------------------------------------------------------------------
def update(clouds, offsets, cfg, G, m, states=None, evidence=None, max_points=None, with_parts=False):
    """one rr_occupancy_update -> int32 [height][width] (`evidence` plus this call; the sums wrap as int32 does).  with_parts: also the
    profile and the per-cell azimuth index under the last scan"""
    ev = np.zeros((cfg.height, cfg.width), np.int64) if evidence is None else np.asarray(evidence, np.int32).astype(np.int64).reshape(cfg.height, cfg.width)
    free2 = profile(clouds, offsets, G, m, max_points)
    n_free, a = free_counts(free2, cfg, G, states)
    out = (ev - m["l_free"] * n_free + m["l_hit"] * hit_counts(clouds, cfg, states, max_points)).astype(np.int32)
    return (out, free2, a) if with_parts else out


def to_map(evidence):
    """rr_occupancy_map: clamp(128 + evidence, 0, 255)"""
    return np.clip(128 + np.asarray(evidence, np.int32).astype(np.int64), 0, 255).astype(np.uint8)


def occ_cfg(m, n_cells):
    return native.occupancy_config(n_cells=n_cells, **m)


# ---- the closed loop of the host and GPU tests: the room of tests/icp_ref.py (14 m x 9 m, the sensor off-centre, 64 azimuths, the 2 strongest
# returns per azimuth) seen from eight poses, on the grid of field_ref's loop (0.25 m cells).  ONE phantom point is injected into ONE scan, in
# the room's interior: the rasteriser makes it a wall, seven scans that look through its cell take it out of the occupancy map again.
LOOP_POSES = [(0.0, 0.0, 0.0), (1.0, 3.0, math.radians(45.0)), (-1.0, 0.5, math.radians(30.0)), (1.5, -0.5, math.radians(-20.0)),
              (-2.0, 1.0, math.radians(75.0)), (2.5, 1.5, math.radians(140.0)), (-3.0, -1.0, math.radians(-100.0)), (0.5, 2.0, math.radians(200.0))]
LOOP_PHANTOM_SCAN = 3
LOOP_PHANTOM_RANGE_BIN, LOOP_PHANTOM_COLUMN = 20, 10                 # in scan 3's own frame: 20.5 bins of 0.0595 m along column 10, 1.2 m out
# the model.  margin_bins: a wall's own cell must not be swept free by the scans that see the wall a little further out in it:
# at least ceil(0.71 * cell / resolution) = ceil(0.71 * 0.25 / 0.0595) = 3 bins (half a cell's diagonal); 5 is used.  l_hit against l_free:
# a wall cell seen in at least half of the eight scans collects >= 4 * l_hit and can lose at most 4 * l_free to the others, so l_hit > l_free
# keeps it.  (3, 2) is what test_occupancy_host.py's loop settled on over the oracle's images; what was tried first is in DESIGN.md §24
LOOP_MODEL = model(l_hit=3, l_free=2, margin_bins=5, max_free_bin=320)


def loop_states():
    p = np.asarray(LOOP_POSES, np.float64)
    return native.se2_states(p[:, 2], p[:, 0], p[:, 1])


def loop_polar():
    import icp_ref
    return polar(icp_ref.LOOP_CELLS, icp_ref.LOOP_ANGLES, resolution=icp_ref.loop_cfg().resolution)


def inject_phantom(clouds, offsets, G):
    """scan LOOP_PHANTOM_SCAN gains one detection, in front of the first one of its column (sorted by bin, the offsets moved up behind it)
    -> (clouds, offsets, the phantom's point)"""
    f, col, b = LOOP_PHANTOM_SCAN, LOOP_PHANTOM_COLUMN, LOOP_PHANTOM_RANGE_BIN
    offs = np.array(offsets, np.uint32).reshape(len(clouds), G.n_angles + 1)
    at = int(offs[f, col])
    assert offs[f, col + 1] == at or clouds[f][at]["bin"] > b        # it is the first of its column
    theta = f32(G.theta_min) + f32((col - G.scroll) % G.n_angles) * f32(G.theta_inc)
    r = f32((b + 0.5) * G.resolution)
    p = np.zeros(1, native.POINT_DTYPE)
    p["x"], p["y"], p["intensity"], p["column"], p["bin"] = r * np.cos(theta), r * np.sin(theta), 200.0, col, b
    out = list(clouds)
    out[f] = np.concatenate([clouds[f][:at], p, clouds[f][at:]])
    offs[f, col + 1:] += 1
    return out, offs, p[0]


def loop_checks(occ_raster, occ_map, clouds_clean, phantom, cfg, states):
    """the three statements of the closed loop that need no GPU -> (the phantom's cell, the wall cells)"""
    inside, index = F.cells(*F.move(f32(phantom["x"]), f32(phantom["y"]), tuple(states[LOOP_PHANTOM_SCAN])), cfg)
    assert bool(inside)
    cell = (int(index) // cfg.width, int(index) % cfg.width)
    assert occ_raster[cell] == 1 and occ_map[cell] < 128, (cell, occ_raster[cell], occ_map[cell])
    seen = np.zeros((cfg.height, cfg.width), np.int64)
    for f, cloud in enumerate(clouds_clean):
        seen += hit_counts([cloud], cfg, states[f:f + 1]) > 0
    walls = seen >= (len(clouds_clean) + 1) // 2
    assert walls.sum() > 20 and np.all(occ_map[walls] > 128), (int(walls.sum()), occ_map[walls].min())
    return cell, walls


# §23's own argmin of the lattice search on the one-scan map (field_ref.LOOP_*_MEASURED: the node 0.2 m, 0.05 m and 0 degrees off pose B);
# test_occupancy_host.py recomputes it on the oracle's images
LOOP_FIELD_NODE = (0.25, 0.25, math.radians(2.0))


def loop_argmin_check(node):
    """statement 3: the argmin on the field of the occupancy map lies within one lattice step of §23's own, in each of x, y and yaw"""
    d = float(node[2]) - LOOP_FIELD_NODE[2]
    dyaw = abs(math.atan2(math.sin(d), math.cos(d)))
    assert abs(float(node[0]) - LOOP_FIELD_NODE[0]) <= F.LOOP_STEP_XY + 1e-9 and abs(float(node[1]) - LOOP_FIELD_NODE[1]) <= F.LOOP_STEP_XY + 1e-9 \
        and dyaw <= F.LOOP_STEP_YAW + 1e-9, tuple(node)
