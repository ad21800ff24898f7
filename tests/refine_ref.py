"""Map refinement of include/radarays_mi355.h (rr_nearest_field, rr_refine_poses) restated in numpy: f32 where the definition says f32 (numpy
rounds every operation and fuses none), Python floats (IEEE f64) for the solve, integers everywhere else.  The GPU tests compare against it
byte for byte; the host tests hold nearest_field (the two-pass construction the kernels use) to nearest_field_brute (the definition itself:
the minimum 64-bit key over the list of occupied cells).  The solve, the normalisation and the cell rule are imported, not restated."""
import math

import numpy as np

import field_ref as F
import icp_ref
from field_ref import cells, move, occupied, points_of, xy_of   # noqa: F401  (cells is the cell rule of the definition)
from icp_ref import normalise, solve
from radarays_ros_amd import native

NONE = native.NEAREST_NONE
DEGENERATE, TRUNCATED = native.ICP_DEGENERATE, native.ICP_TRUNCATED


def nearest_field(occ, cfg, threshold=1):
    """the two-pass construction.  Pass A, per column: the signed vertical offset dy to the column's nearest occupied cell (jy = iy + dy; a
    tie between above and below goes to the lower jy), saturated at +max_dist (an upward and a downward scan).  Pass B, per row: the minimum
    over |dx| < max_dist of the key ((dx^2 + dy^2) << 32) | ((iy + dy) * W + ix + dx) in 64 bits, the index part wrapped to 32 bits; a cell
    beyond the row's end counts as saturated.  NONE where the minimal d2 is not below cap2."""
    H, W, md = cfg.height, cfg.width, cfg.max_dist
    o = occupied(occ, threshold).reshape(H, W)
    off = np.zeros((H, W), np.int64)
    d = np.full(W, md, np.int64)
    for iy in range(H):
        d = np.where(o[iy], 0, np.minimum(d + 1, md))
        off[iy] = np.where(d < md, -d, md)
    d = np.full(W, md, np.int64)
    for iy in range(H - 1, -1, -1):
        d = np.where(o[iy], 0, np.minimum(d + 1, md))
        off[iy] = np.where((off[iy] == md) | (d < -off[iy]), d, off[iy])     # a tie (d == -off) keeps the lower jy
    pad = np.full((H, W + 2 * md), md, np.int64)
    pad[:, md:md + W] = off
    iy, ix = np.mgrid[0:H, 0:W].astype(np.int64)
    best = np.full((H, W), np.iinfo(np.uint64).max, np.uint64)
    for dx in range(1 - md, md):
        dy = pad[:, md + dx:md + dx + W]
        d2 = (dx * dx + dy * dy).astype(np.uint64)
        index = (((iy + dy) * W + ix + dx) & 0xFFFFFFFF).astype(np.uint64)
        best = np.minimum(best, (d2 << np.uint64(32)) | index)
    return np.where((best >> np.uint64(32)) < np.uint64(md * md), best & np.uint64(0xFFFFFFFF), np.uint64(NONE)).astype(np.uint32)


def nearest_field_brute(occ, cfg, threshold=1, chunk=1 << 21):
    """the definition: over the list of occupied cells the minimum of (d2 << 32) | (jy * W + jx); its index where d2 < cap2, else NONE"""
    H, W = cfg.height, cfg.width
    cap2 = cfg.max_dist * cfg.max_dist
    jy, jx = np.nonzero(occupied(occ, threshold).reshape(H, W))
    out = np.full(H * W, NONE, np.uint32)
    if len(jy):
        lin = (jy * W + jx).astype(np.int64)
        iy, ix = np.divmod(np.arange(H * W, dtype=np.int64), W)
        step = max(1, chunk // len(jy))
        for a in range(0, H * W, step):
            d2 = (ix[a:a + step, None] - jx[None, :]) ** 2 + (iy[a:a + step, None] - jy[None, :]) ** 2
            key = ((d2 << 32) | lin[None, :]).min(axis=1)            # below 2^57: int64 holds it
            out[a:a + step] = np.where((key >> 32) < cap2, key & 0xFFFFFFFF, NONE).astype(np.uint32)
    return out.reshape(H, W)


def nearest_d2(nearest, cfg):
    """(the mask nearest != NONE, the squared distance in cells from every cell to the cell its entry names; 0 where the mask is False)"""
    H, W = cfg.height, cfg.width
    k = np.asarray(nearest, np.uint32).reshape(H, W).astype(np.int64)
    some = k != NONE
    iy, ix = np.mgrid[0:H, 0:W]
    jy, jx = np.divmod(np.where(some, k, 0), W)
    return some, np.where(some, (ix - jx) ** 2 + (iy - jy) ** 2, 0)


def pass_sums(x, y, states, near_flat, cfg):
    """one pass of every state of float64 [n][4] over the scan -> int64 [n][8], the sums in the order of icp_ref.SUMS"""
    W = cfg.width
    cell, x0, y0 = np.float32(cfg.cell), np.float32(cfg.x0), np.float32(cfg.y0)
    half, s256 = np.float32(0.5), np.float32(256.0)
    st = np.asarray(states, np.float64).reshape(-1, 4)
    px, py = move(x[None, :], y[None, :], (st[:, 0:1], st[:, 1:2], st[:, 2:3], st[:, 3:4]))
    inside, index = cells(px, py, cfg)
    k = near_flat[index]
    jy, jx = np.divmod(k, W)
    iy, ix = np.divmod(index, W)
    matched = inside & (k != NONE) & ((ix - jx) ** 2 + (iy - jy) ** 2 <= cfg.gate * cfg.gate)
    qx = x0 + (jx.astype(np.float32) + half) * cell                   # the cell-centre expression of the occupancy grid
    qy = y0 + (jy.astype(np.float32) + half) * cell
    zero = np.float32(0)
    quant = lambda v: np.rint(np.where(matched, v, zero) * s256).astype(np.int64)   # noqa: E731
    Px, Py, Qx, Qy = quant(px), quant(py), quant(qx), quant(qy)
    tot = lambda v: np.where(matched, v, 0).sum(axis=1, dtype=np.int64)             # noqa: E731
    return np.stack([matched.sum(axis=1, dtype=np.int64), tot(Px), tot(Py), tot(Qx), tot(Qy), tot(Px * Qx + Py * Qy), tot(Px * Qy - Py * Qx),
                     tot((Px - Qx) ** 2 + (Py - Qy) ** 2)], axis=1)


def refine(points, init, nearest, cfg, iterations=10, max_points=None, chunk=256):
    """one scan from the initial states [n][4] against the table -> ICP_DTYPE [n].  A scan longer than max_points is cut and flagged."""
    x, y = xy_of(points)
    flags0 = 0
    if max_points is not None and len(x) > max_points:
        x, y, flags0 = x[:max_points], y[:max_points], TRUNCATED
    near_flat = np.asarray(nearest, np.uint32).reshape(-1).astype(np.int64)
    init = np.asarray(init, np.float64).reshape(-1, 4)
    n = len(init)
    states, flags = [], []
    for h in range(n):
        state, deg = normalise(init[h])
        states.append(state)
        flags.append(flags0 | deg)
    recs = np.zeros(n, native.ICP_DTYPE)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        for _ in range(iterations):
            sums = pass_sums(x, y, np.array(states[a:b], np.float64), near_flat, cfg)
            for h in range(a, b):
                states[h], deg = solve(states[h], tuple(int(v) for v in sums[h - a]))
                if deg:
                    flags[h] |= DEGENERATE
        sums = pass_sums(x, y, np.array(states[a:b], np.float64), near_flat, cfg)
        for h in range(a, b):
            c, s, tx, ty = states[h]
            recs[h] = (c, s, tx, ty, int(sums[h - a][7]), int(sums[h - a][0]), flags[h])
    return recs


def cell_centres(index, cfg):
    """the f32 centres of the cells with these linear indices, as [m][2]"""
    jy, jx = np.divmod(np.asarray(index, np.int64), cfg.width)
    cell, half = np.float32(cfg.cell), np.float32(0.5)
    return np.stack([np.float32(cfg.x0) + (jx.astype(np.float32) + half) * cell, np.float32(cfg.y0) + (jy.astype(np.float32) + half) * cell], axis=1)


# ---- the cases of the transform that the host and the GPU tests share ----------------------------------------------------------------
MAX_DISTS = (1, 2, 16, 255)
HEIGHTS = (1, 2, 67)


def grid_list(row_tile):
    """(width, height): 1 x 1, 1 x N, N x 1, and widths at the row pass's tile and one to either side of it under heights 1, 2 and 67"""
    t = min(row_tile, native.FIELD_MAX_SIDE - 1)
    return [(1, 1), (1, 37), (37, 1)] + [(w, h) for w in (t - 1, t, t + 1) for h in HEIGHTS]


def map_list(width, height):
    """name -> uint8 [height][width] holding 0 and 1"""
    H, W = height, width
    rs = np.random.RandomState(7000 * H + W)
    maps = {"empty": np.zeros((H, W), np.uint8), "full": np.ones((H, W), np.uint8)}
    for name, (iy, ix) in (("corner00", (0, 0)), ("corner01", (0, W - 1)), ("corner10", (H - 1, 0)), ("corner11", (H - 1, W - 1))):
        maps[name] = np.zeros((H, W), np.uint8)
        maps[name][iy, ix] = 1
    for pitch in (2, 4):          # equidistant ties across columns, across rows and diagonally
        maps["lattice%d" % pitch] = np.zeros((H, W), np.uint8)
        maps["lattice%d" % pitch][::pitch, ::pitch] = 1
    maps["random1"] = (rs.random_sample((H, W)) < 0.01).astype(np.uint8)
    maps["random30"] = (rs.random_sample((H, W)) < 0.30).astype(np.uint8)
    return maps


def grid_cfg(width, height, max_dist, gate=0, cell=0.5, x0=0.0, y0=0.0):
    return native.field_config(width, height, cell, x0, y0, max_dist, min(gate, max_dist))


# ---- the closed loop of the host and GPU tests: the room, grid, scan and poses of tests/icp_ref.py and tests/field_ref.py.  The map is the
# rasterised cloud of pose A; B's scan is refined from A's own planar state -- the guess the scan matcher starts from, 2 degrees and 0.492 m
# off the truth, which is B's planar pose in the map.
LOOP_GATE, LOOP_ITERATIONS = 4, 10                                   # cells; the first values tried
LOOP_GUESS_YAW, LOOP_GUESS_T = math.radians(2.0), math.hypot(0.45, 0.2)


def loop_field_cfg():
    g = F.loop_field_cfg()
    return native.field_config(g.width, g.height, g.cell, g.x0, g.y0, F.LOOP_MAX_DIST, LOOP_GATE)


def loop_guess():
    return native.se2_states(icp_ref.LOOP_A[2], icp_ref.LOOP_A[0], icp_ref.LOOP_A[1])


def loop_errors(rec):
    """(|yaw error| in radians, translation error in metres) of a record against the truth, pose B"""
    return icp_ref.loop_errors(rec)


# what the restatement gives on the oracle's images (test_refine_host.py measures, prints and pins it); the bound of the tests is twice the
# figure in each, the scan matcher's rule
LOOP_YAW_MEASURED, LOOP_T_MEASURED = math.radians(1.2520), 0.2751
LOOP_YAW_BOUND, LOOP_T_BOUND = 2 * LOOP_YAW_MEASURED, 2 * LOOP_T_MEASURED
