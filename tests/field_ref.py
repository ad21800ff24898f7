"""The likelihood field of include/radarays_mi355.h (rr_rasterize_points, rr_distance_field, rr_score_poses) restated in numpy: f32 where the
definition says f32 (numpy rounds every operation and fuses none), integers everywhere else.  The GPU tests compare against it bit for bit;
the host tests hold distance_field (the two-pass construction the kernels use) to distance_field_brute (the definition itself: the minimum
over the list of occupied cells) and, where scipy is installed, to scipy's Euclidean distance transform."""
import math

import numpy as np

from radarays_ros_amd import native


def xy_of(cloud):
    """a POINT_DTYPE array, or anything [m][2] -> (x, y) as float32 arrays"""
    c = np.asarray(cloud)
    if c.dtype == native.POINT_DTYPE:
        return c["x"].astype(np.float32), c["y"].astype(np.float32)
    c = np.asarray(c, np.float32).reshape(-1, 2)
    return c[:, 0].copy(), c[:, 1].copy()


def points_of(xy):
    """[m][2] -> POINT_DTYPE with z, intensity, column and bin the field must ignore"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    p = np.zeros(len(xy), native.POINT_DTYPE)
    p["x"], p["y"] = xy[:, 0], xy[:, 1]
    p["z"], p["intensity"], p["column"], p["bin"] = -3.5, 99.0, 0xFFFFFFF1, 654321
    return p


def move(x, y, state):
    """step 1 of the scan matcher: (c, s, tx, ty), each rounded to f32 -> px = (cf*x - sf*y) + txf, py = (sf*x + cf*y) + tyf.  x, y and the
    state's parts broadcast against each other"""
    with np.errstate(invalid="ignore", over="ignore"):
        cf, sf, txf, tyf = (np.asarray(v).astype(np.float32) for v in state)
        return (cf * x - sf * y) + txf, (sf * x + cf * y) + tyf


def cells(px, py, cfg):
    """the cell rule: (IN GRID mask, linear index iy * width + ix; 0 where the mask is False)"""
    cell, x0, y0 = np.float32(cfg.cell), np.float32(cfg.x0), np.float32(cfg.y0)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (px - x0) / cell
        v = (py - y0) / cell
        inside = (u >= np.float32(0)) & (u < np.float32(cfg.width)) & (v >= np.float32(0)) & (v < np.float32(cfg.height))     # False for NaN, +-inf
        ix = np.where(inside, np.floor(u), 0).astype(np.int64)
        iy = np.where(inside, np.floor(v), 0).astype(np.int64)
    return inside, iy * cfg.width + ix


def rasterize(clouds, cfg, states=None, occ=None, max_points=None):
    """clouds (a list of [m][2] or POINT_DTYPE arrays) under their states (float64 [n][4] or None) -> uint8 [height][width]: `occ` (or an
    empty grid) with a 1 in the cell of every point that is IN GRID.  A cloud longer than max_points loses its tail."""
    out = np.zeros((cfg.height, cfg.width), np.uint8) if occ is None else np.array(occ, np.uint8).reshape(cfg.height, cfg.width)
    flat = out.reshape(-1)
    for f, cloud in enumerate(clouds):
        x, y = xy_of(cloud)
        if max_points is not None:
            x, y = x[:max_points], y[:max_points]
        state = (1.0, 0.0, 0.0, 0.0) if states is None else tuple(np.asarray(states, np.float64)[f])
        px, py = move(x, y, state)
        inside, index = cells(px, py, cfg)
        flat[index[inside]] = 1
    return out


def occupied(occ, threshold):
    return np.asarray(occ, np.uint8) >= threshold


def distance_field(occ, cfg, threshold=1):
    """the two-pass construction.  Pass A, per column: g = the vertical distance to the nearest occupied cell, saturated at max_dist (an
    upward and a downward scan).  Pass B, per row: min over |dx| <= max_dist of dx*dx + g[ix + dx]^2, clamped to cap2; a cell beyond the
    row's end counts as saturated."""
    H, W, md = cfg.height, cfg.width, cfg.max_dist
    o = occupied(occ, threshold).reshape(H, W)
    g = np.zeros((H, W), np.int64)
    d = np.full(W, md, np.int64)
    for iy in range(H):
        d = np.where(o[iy], 0, np.minimum(d + 1, md))
        g[iy] = d
    d = np.full(W, md, np.int64)
    for iy in range(H - 1, -1, -1):
        d = np.where(o[iy], 0, np.minimum(d + 1, md))
        g[iy] = np.minimum(g[iy], d)
    cap2 = md * md
    g2 = np.full((H, W + 2 * md), cap2, np.int64)
    g2[:, md:md + W] = g * g
    best = np.full((H, W), cap2, np.int64)
    for dx in range(-md, md + 1):
        best = np.minimum(best, dx * dx + g2[:, md + dx:md + dx + W])
    return best.astype(np.uint16)


def distance_field_brute(occ, cfg, threshold=1, chunk=1 << 22):
    """the definition: min(cap2, min over the occupied cells (jx, jy) of (ix-jx)^2 + (iy-jy)^2), taken over the list of occupied cells"""
    H, W = cfg.height, cfg.width
    cap2 = cfg.max_dist * cfg.max_dist
    jy, jx = np.nonzero(occupied(occ, threshold).reshape(H, W))
    out = np.full(H * W, cap2, np.int64)
    if len(jy):
        iy, ix = np.divmod(np.arange(H * W, dtype=np.int64), W)
        step = max(1, chunk // len(jy))
        for a in range(0, H * W, step):
            d2 = (ix[a:a + step, None] - jx[None, :]) ** 2 + (iy[a:a + step, None] - jy[None, :]) ** 2
            out[a:a + step] = np.minimum(cap2, d2.min(axis=1))
    return out.reshape(H, W).astype(np.uint16)


def score(points, states, field, cfg, max_points=None, chunk=256):
    """one scan against float32 states [n][4] -> FIELD_DTYPE [n]"""
    x, y = xy_of(points)
    if max_points is not None:
        x, y = x[:max_points], y[:max_points]
    st = np.ascontiguousarray(states, np.float32).reshape(-1, 4)
    flat = np.asarray(field, np.uint16).reshape(-1).astype(np.int64)
    cap2, gate2 = cfg.max_dist * cfg.max_dist, cfg.gate * cfg.gate
    recs = np.zeros(len(st), native.FIELD_DTYPE)
    for a in range(0, len(st), chunk):
        s = st[a:a + chunk]
        px, py = move(x[None, :], y[None, :], (s[:, 0:1], s[:, 1:2], s[:, 2:3], s[:, 3:4]))
        inside, index = cells(px, py, cfg)
        d = np.where(inside, flat[index], cap2)
        recs["sum_d2"][a:a + chunk] = d.sum(axis=1)
        recs["n_in"][a:a + chunk] = inside.sum(axis=1)
        recs["n_hit"][a:a + chunk] = (inside & (d <= gate2)).sum(axis=1)
    return recs


# ---- the cases of the transform that the host and the GPU tests share: every grid x every map x every max_dist -----------------------
MAX_DISTS = (1, 2, 7, 255)


def grid_list(row_tile):
    """(width, height): the degenerate and odd grids, and widths and heights at the row pass's tile and one to either side of it"""
    t = min(row_tile, native.FIELD_MAX_SIDE - 1)
    return [(1, 1), (1, 37), (37, 1), (33, 65), (64, 64), (t - 1, t + 1), (t, t), (t + 1, t - 1)]


def map_list(width, height):
    """name -> uint8 [height][width] holding 0 and 1"""
    H, W = height, width
    rs = np.random.RandomState(1000 * H + W)
    maps = {"empty": np.zeros((H, W), np.uint8), "full": np.ones((H, W), np.uint8)}
    for name, (iy, ix) in (("corner00", (0, 0)), ("corner01", (0, W - 1)), ("corner10", (H - 1, 0)), ("corner11", (H - 1, W - 1)),
                           ("centre", (H // 2, W // 2))):
        maps[name] = np.zeros((H, W), np.uint8)
        maps[name][iy, ix] = 1
    # two cells equidistant from a third: the cell between them sees both at the same distance (on a grid too small for that, what fits)
    eq = np.zeros((H, W), np.uint8)
    eq[0, 0] = 1
    eq[min(4, H - 1), min(2, W - 1)] = 1                              # (2, 4) and ...
    eq[min(2, H - 1), min(4, W - 1)] = 1                              # ... (4, 2) are equally far from (0, 0), and (3, 3) from both
    maps["equidistant"] = eq
    maps["random1"] = (rs.random_sample((H, W)) < 0.01).astype(np.uint8)
    maps["random50"] = (rs.random_sample((H, W)) < 0.5).astype(np.uint8)
    return maps


def grid_cfg(width, height, max_dist, gate=0, cell=0.5, x0=0.0, y0=0.0):
    return native.field_config(width, height, cell, x0, y0, max_dist, min(gate, max_dist))


# ---- the closed loop of the host and GPU tests: the asymmetric box room of tests/icp_ref.py (same scene, 64 azimuths, the 2 strongest
# returns per azimuth).  The map is the cloud of pose A under A's own planar pose, at 0.25 m cells; the scan is taken at pose B = A moved by
# (0.45 m, 0.2 m, 2 degrees); the hypotheses are the lattice around A of +-1 m in steps of 0.25 m and +-4 degrees in steps of 1 degree:
# 9 x 9 x 9 = 729.  The truth is B's planar pose in the map.
LOOP_CELL = 0.25
LOOP_MAX_DIST, LOOP_GATE = 16, 2                                      # saturate at 4 m, a HIT within 0.5 m
LOOP_HALF_XY, LOOP_STEP_XY, LOOP_HALF_YAW, LOOP_STEP_YAW = 1.0, 0.25, math.radians(4.0), math.radians(1.0)


def loop_field_cfg():
    """the room is 14 m x 9 m from (-8, -3); the grid leaves 2 m around it: 72 x 52 cells from (-10, -5)"""
    return native.field_config(72, 52, LOOP_CELL, -10.0, -5.0, LOOP_MAX_DIST, LOOP_GATE)


def loop_lattice():
    import icp_ref
    return native.pose_lattice(icp_ref.LOOP_A, LOOP_HALF_XY, LOOP_STEP_XY, LOOP_HALF_YAW, LOOP_STEP_YAW)


def loop_map_state():
    import icp_ref
    return native.se2_states(icp_ref.LOOP_A[2], icp_ref.LOOP_A[0], icp_ref.LOOP_A[1])


def loop_errors(xyz_node):
    """(|x error|, |y error| in metres, |yaw error| in radians) of a lattice node against the truth, pose B"""
    import icp_ref
    d = float(xyz_node[2]) - icp_ref.LOOP_B[2]
    return abs(float(xyz_node[0]) - icp_ref.LOOP_B[0]), abs(float(xyz_node[1]) - icp_ref.LOOP_B[1]), abs(math.atan2(math.sin(d), math.cos(d)))


# what the restatement gives on the oracle's images (test_field_host.py measures, prints and pins it): the argmin is the node
# (0.25 m, 0.25 m, 2 degrees), alone at sum_d2 = 100 (the centre node: 190), so its distance from the truth is 0.2 m in x, 0.05 m in y and
# nothing in yaw.  The node nearest the truth, (0.5, 0.25, 2 degrees), comes third at 105: with 128 points about 1 m apart on the walls
# and cells of 0.25 m the landscape is flat within one lattice step, which is the margin the GPU test allows on top of this figure
LOOP_X_MEASURED, LOOP_Y_MEASURED, LOOP_YAW_MEASURED = 0.2, 0.05, 0.0
