"""The scan matcher of include/radarays_mi355.h (rr_register_points) restated in numpy: f32 where the definition says f32 (numpy rounds every
operation and fuses none), Python floats (IEEE f64, correctly rounded + - * / sqrt) for the solve, Python ints for the sums.  The GPU tests
compare against it bit for bit; the host tests hold it to hand-worked cases."""
import math

import numpy as np

from radarays_ros_amd import native

NONE = native.ICP_NONE
DEGENERATE, TRUNCATED = native.ICP_DEGENERATE, native.ICP_TRUNCATED
RANGE = np.float32(8192.0)
SUMS = ("N", "SPx", "SPy", "SQx", "SQy", "Sdot", "Scross", "Ssse")


def xy_of(cloud):
    """a POINT_DTYPE array, or anything [m][2] -> (x, y) as float32 arrays"""
    c = np.asarray(cloud)
    if c.dtype == native.POINT_DTYPE:
        return c["x"].astype(np.float32), c["y"].astype(np.float32)
    c = np.asarray(c, np.float32).reshape(-1, 2)
    return c[:, 0].copy(), c[:, 1].copy()


def points_of(xy):
    """[m][2] -> POINT_DTYPE with z, intensity, column and bin the matcher must ignore"""
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    p = np.zeros(len(xy), native.POINT_DTYPE)
    p["x"], p["y"] = xy[:, 0], xy[:, 1]
    p["z"], p["intensity"], p["column"], p["bin"] = 7.5, 200.0, 0xFFFFFFF0, 123456
    return p


def normalise(init):
    """one initial state -> ((c, s, tx, ty) as Python floats, flags)"""
    c, s, tx, ty = (float(v) for v in init)
    h = math.sqrt(c * c + s * s)                                      # (inf and NaN pass through sqrt)
    if not (h > 0.0 and math.isfinite(h)):
        return (1.0, 0.0, 0.0, 0.0), DEGENERATE
    return (c / h, s / h, tx, ty), 0


def correspondence_pass(sx, sy, tx, ty, state, gate2, chunk=256):
    """one pass: (j* uint32 [m] with NONE for an unmatched point, the eight sums as Python ints in the order of SUMS)"""
    cf, sf, txf, tyf = (np.float32(v) for v in state)
    with np.errstate(invalid="ignore", over="ignore"):
        px = (cf * sx - sf * sy) + txf
        py = (sf * sx + cf * sy) + tyf
        ok_t = (np.abs(tx) < RANGE) & (np.abs(ty) < RANGE)           # False for NaN and infinities
        inf = np.float32(np.inf)
        qx, qy = np.where(ok_t, tx, inf), np.where(ok_t, ty, inf)
        m = len(sx)
        best = np.full(m, inf, np.float32)
        j = np.full(m, NONE, np.uint32)
        if len(tx):
            for a in range(0, m, chunk):
                dx = px[a:a + chunk, None] - qx[None, :]
                dy = py[a:a + chunk, None] - qy[None, :]
                d2 = dx * dx + dy * dy
                d2 = np.where(np.isnan(d2), inf, d2)                 # a NaN never wins
                k = np.argmin(d2, axis=1)                            # the first of equal minima: the lower index
                b = d2[np.arange(len(k)), k]
                won = b < inf                                        # `d2 < best` from best = +inf
                best[a:a + chunk] = np.where(won, b, inf)
                j[a:a + chunk] = np.where(won, k, NONE).astype(np.uint32)
        matched = (np.abs(px) < RANGE) & (np.abs(py) < RANGE) & (j != NONE) & (best <= gate2)
        j = np.where(matched, j, NONE).astype(np.uint32)
        jm = j[matched].astype(np.int64)
        s256 = np.float32(256.0)
        Px, Py = np.rint(px[matched] * s256).astype(np.int64), np.rint(py[matched] * s256).astype(np.int64)
        Qx, Qy = np.rint(tx[jm] * s256).astype(np.int64), np.rint(ty[jm] * s256).astype(np.int64)
    tot = lambda v: int(np.sum(v, dtype=np.int64))   # noqa: E731  (no sum leaves int64: at most 65,536 terms below 2^45)
    sums = (int(matched.sum()), tot(Px), tot(Py), tot(Qx), tot(Qy), tot(Px * Qx + Py * Qy), tot(Px * Qy - Py * Qx),
            tot((Px - Qx) ** 2 + (Py - Qy) ** 2))
    return j, sums


def solve(state, sums):
    """one solve: (the new state, degenerate?)"""
    c, s, tx, ty = state
    Ni = sums[0]
    N, SPx, SPy, SQx, SQy, Sdot, Scross = (float(v) for v in sums[:7])
    A = N * Sdot - (SPx * SQx + SPy * SQy)
    B = N * Scross - (SPx * SQy - SPy * SQx)
    h = math.sqrt(A * A + B * B)
    if Ni < 2 or not h > 0.0:
        return state, True
    dc, ds = A / h, B / h
    mpx, mpy, mqx, mqy = (SPx / N) / 256.0, (SPy / N) / 256.0, (SQx / N) / 256.0, (SQy / N) / 256.0
    dtx = mqx - (dc * mpx - ds * mpy)
    dty = mqy - (ds * mpx + dc * mpy)
    c1 = dc * c - ds * s
    s1 = ds * c + dc * s
    tx1 = (dc * tx - ds * ty) + dtx
    ty1 = (ds * tx + dc * ty) + dty
    n = math.sqrt(c1 * c1 + s1 * s1)
    return (c1 / n, s1 / n, tx1, ty1), False


def register(sources, target, init=None, gate=1.0, iterations=10, max_points=None, max_tgt=None):
    """n source clouds against one target -> (records ICP_DTYPE [n], states float64 [iterations + 1][n][4]: the state each pass ran at,
    a list of n uint32 arrays: the last pass's j* per point).  A cloud longer than max_points / max_tgt is cut and flagged."""
    n = len(sources)
    tx, ty = xy_of(target)
    t_trunc = max_tgt is not None and len(tx) > max_tgt
    if t_trunc:
        tx, ty = tx[:max_tgt], ty[:max_tgt]
    g = np.float32(gate)
    gate2 = g * g
    recs = np.zeros(n, native.ICP_DTYPE)
    states = np.zeros((iterations + 1, n, 4), np.float64)
    corr = []
    for f in range(n):
        sx, sy = xy_of(sources[f])
        flags = 0
        if max_points is not None and len(sx) > max_points:
            sx, sy, flags = sx[:max_points], sy[:max_points], TRUNCATED
        if t_trunc:
            flags |= TRUNCATED
        state = (1.0, 0.0, 0.0, 0.0)
        if init is not None:
            state, deg = normalise(init[f])
            flags |= deg
        for it in range(iterations):
            states[it, f] = state
            _, sums = correspondence_pass(sx, sy, tx, ty, state, gate2)
            state, deg = solve(state, sums)
            if deg:
                flags |= DEGENERATE
        states[iterations, f] = state
        j, sums = correspondence_pass(sx, sy, tx, ty, state, gate2)
        recs[f] = (state[0], state[1], state[2], state[3], sums[7], sums[0], flags)
        corr.append(j)
    return recs, states, corr


def yaw_of(rec):
    return np.arctan2(rec["s"], rec["c"])


def compose_inverse(pose_xyyaw, rec):
    """the corrected planar pose X_h * T^-1 of a hypothesis X_h = (x, y, yaw) whose cloud the record's T maps onto the target's"""
    x, y, yaw = pose_xyyaw
    c, s, tx, ty = float(rec["c"]), float(rec["s"]), float(rec["tx"]), float(rec["ty"])
    ix, iy = -(c * tx + s * ty), -(-s * tx + c * ty)                  # T^-1 = (R^T, -R^T t)
    return x + math.cos(yaw) * ix - math.sin(yaw) * iy, y + math.sin(yaw) * ix + math.cos(yaw) * iy, yaw - math.atan2(s, c)


# ---- the closed loop of the host and GPU tests: a closed box room that is not symmetric, 14 m x 9 m x 5 m with the sensor off-centre,
# 64 azimuths; pose B is 0.49 m and 2 degrees away from pose A.  Both clouds are the 2 strongest returns per azimuth; B's cloud is
# registered onto A's from the identity guess.  The truth is T = A^-1 B; A is the map's origin, so T is B's planar pose itself.
LOOP_LO, LOOP_HI = (-8.0, -3.0, -2.0), (6.0, 6.0, 3.0)
LOOP_ANGLES, LOOP_CELLS, LOOP_SAMPLES = 64, 320, 50
LOOP_A, LOOP_B = (0.0, 0.0, 0.0), (0.45, 0.2, math.radians(2.0))      # (x, y, yaw)
LOOP_DET = dict(method=1, k=2, min_intensity=1)
LOOP_GATE, LOOP_ITERATIONS = 1.0, 10
# what the restatement gives on the oracle's images (test_icp_host.py measures and prints it): point-to-point matching of walls sampled
# once per azimuth slides along them, so the residual is a fraction of the 1 m point spacing, not of the 1/256 m quantisation step
LOOP_YAW_MEASURED, LOOP_T_MEASURED = math.radians(0.456), 0.1817
LOOP_YAW_BOUND, LOOP_T_BOUND = 2 * LOOP_YAW_MEASURED, 2 * LOOP_T_MEASURED


def loop_scene():
    from radarays_ros_amd import scenes
    v, f = scenes._box_tris(LOOP_LO, LOOP_HI)
    return {"verts": v, "faces": f, "face_object_id": np.zeros(len(f), np.uint32), "object_materials": [1]}


def loop_cfg():
    from radarays_ros_amd import params
    return params.kaist_preset(n_reflections=1, n_samples=LOOP_SAMPLES, ambient_noise=0, signal_denoising=0, n_cells=LOOP_CELLS)


def loop_pose(xyyaw):
    from radarays_ros_amd import scenes
    return scenes.yaw_pose(xyyaw[0], xyyaw[1], 0.0, xyyaw[2])


def loop_errors(rec, truth=LOOP_B):
    """(|yaw error| in radians, translation error in metres) of a record against the true transform (x, y, yaw)"""
    d = float(yaw_of(rec)) - truth[2]
    d = abs(math.atan2(math.sin(d), math.cos(d)))
    return d, math.hypot(float(rec["tx"]) - truth[0], float(rec["ty"]) - truth[1])
