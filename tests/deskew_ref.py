"""numpy restatement of the sweep compensation (include/radarays_mi355.h, rr_deskew.hip): the record table, the compensated
points and the compensated Cartesian image.

The definitions are this build's own; these functions state them a second time, in float32 with one rounding per operation and
nothing fused, in the operation order of the header (q_mul / q_rot in the term order of rr_device.h, as tests/dynamic_ref.py
builds them).  `dtype` lets the Cartesian image be recomputed in float64, which the tests use to see how many pixels of their
inputs sit on a rounding boundary."""
import numpy as np

from radarays_ros_amd.native import POINT_DTYPE, SWEEP_DTYPE


def q_mul(a, b):
    """rr_device.h q_mul (Hamilton product), a, b [..., 4] -> [..., 4]"""
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], -1)


def q_conj(q):
    return q * np.array([-1, -1, -1, 1], q.dtype)


def q_rot(q, v):
    """rr_device.h q_rot in its term order; q [..., 4], v [..., 3] -> [..., 3]"""
    qx, qy, qz, qw = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    vx, vy, vz = v[..., 0], v[..., 1], v[..., 2]
    tx = qw * vx + qy * vz - qz * vy
    ty = qw * vy - qx * vz + qz * vx
    tz = qw * vz + qx * vy - qy * vx
    tw = q.dtype.type(0.0) - qx * vx - qy * vy - qz * vz
    cx, cy, cz, cw = -qx, -qy, -qz, qw
    rx = tw * cx + tx * cw + ty * cz - tz * cy
    ry = tw * cy - tx * cz + ty * cw + tz * cx
    rz = tw * cz + tx * cy - ty * cx + tz * cw
    return np.stack([rx, ry, rz], -1)


def v_dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def sweep_table(az_poses, ref_poses, sensor_vel=None, gain=0.0, theta_min=0.0, theta_inc=-2 * np.pi / 400):
    """az_poses [n][A][7], ref_poses [n][7], sensor_vel [n][3] or None -> SWEEP_DTYPE [n][A]"""
    f32 = np.float32
    az = np.asarray(az_poses, f32)
    ref = np.asarray(ref_poses, f32).reshape(-1, 7)
    if az.ndim == 2:
        az = az[None]
    n, A = az.shape[:2]
    q_a, t_a = az[..., :4], az[..., 4:]
    q_ref, t_ref = ref[:, None, :4], ref[:, None, 4:]
    out = np.zeros((n, A), SWEEP_DTYPE)
    out["q"] = q_mul(q_conj(np.broadcast_to(q_ref, q_a.shape)), q_a)
    out["t"] = q_rot(q_conj(np.broadcast_to(q_ref, q_a.shape)), t_a - t_ref)
    if sensor_vel is not None and f32(gain) != 0:
        theta = f32(theta_min) + np.arange(A, dtype=f32) * f32(theta_inc)
        d = np.stack([np.cos(theta), np.sin(theta), np.zeros(A, f32)], -1).astype(f32)
        u = q_rot(q_a, np.broadcast_to(d[None], (n, A, 3)))
        v_s = np.asarray(sensor_vel, f32).reshape(n, 1, 3)
        v_r = -(v_dot(np.broadcast_to(v_s, u.shape), u))
        out["dr"] = f32(gain) * v_r
    return out


def compensate_points(points, table, scroll=0, resolution=0.0438):
    """one frame: points POINT_DTYPE [m], table SWEEP_DTYPE [A] -> POINT_DTYPE [m]"""
    f32 = np.float32
    pts = np.asarray(points)
    A = len(table)
    out = pts.copy()
    a = (pts["column"].astype(np.int64) - int(scroll)) % A
    rec = table[a]
    r = ((pts["bin"].astype(np.float64) + 0.5) * float(resolution)).astype(f32)
    rc = r - rec["dr"]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        p = np.stack([pts["x"], pts["y"], pts["z"]], -1) * (rc / r)[:, None]
        o = q_rot(rec["q"], p.astype(f32)) + rec["t"]
    bad = ~((rc > 0) & np.isfinite(rc)) | (pts["column"] >= A)
    o[bad] = np.nan
    out["x"], out["y"], out["z"] = o[:, 0], o[:, 1], o[:, 2]
    return out


def cartesian_sweep(img, table, width, pixel_size, bilinear=True, iterations=2, scroll=0, theta_min=0.0, theta_inc=-2 * np.pi / 400,
                    resolution=0.0438, dtype=np.float32):
    """one polar image [n_cells][n_angles] and its records SWEEP_DTYPE [n_angles] -> uint8 [width][width] in the reference frame"""
    img = np.asarray(img)
    N, A = img.shape
    ft = np.dtype(dtype).type
    cc = ft(width - 1) * ft(0.5)
    ii, jj = np.meshgrid(np.arange(width, dtype=dtype), np.arange(width, dtype=dtype), indexing="ij")
    P = np.stack([(cc - ii) * ft(np.float32(pixel_size)), (cc - jj) * ft(np.float32(pixel_size)), np.zeros_like(ii)], -1)
    na = ft(A)
    th_min, th_inc, res = ft(np.float32(theta_min)), ft(np.float32(theta_inc)), ft(np.float32(resolution))
    tq, tt, tdr = table["q"].astype(dtype), table["t"].astype(dtype), table["dr"].astype(dtype)

    def az_coord(phi):
        u = np.fmod((phi - th_min) / th_inc, na)
        u = np.where(u < 0, u + na, u).astype(dtype)
        u = np.where(u >= na, u - na, u).astype(dtype)
        return np.where((u >= 0) & (u < na), u, ft(0.0)).astype(dtype)

    def nearest(u):
        return np.rint(u).astype(np.int64) % A

    u = az_coord(np.arctan2(P[..., 1], P[..., 0]))
    a = nearest(u)
    Q, dr = P, np.zeros_like(ii)
    for _ in range(int(iterations)):
        Q = q_rot(q_conj(tq[a]), P - tt[a])
        dr = tdr[a]
        u = az_coord(np.arctan2(Q[..., 1], Q[..., 0]))
        a = nearest(u)
    rho = np.sqrt(v_dot(Q, Q))
    rho_m = rho + dr
    with np.errstate(invalid="ignore"):
        v = rho_m / res - ft(0.5)
        outside = ~(v <= ft(N) - ft(0.5)) | ~((rho_m >= 0) & np.isfinite(rho_m))
    v = np.where(outside, ft(0.0), np.maximum(v, ft(0.0))).astype(dtype)

    def z(b, az):
        return img[np.clip(b, 0, N - 1), (az + int(scroll) % A) % A].astype(dtype)

    if not bilinear:
        out = z(np.minimum(np.rint(v).astype(np.int64), N - 1), nearest(u))
    else:
        a0 = np.minimum(np.floor(u).astype(np.int64), A - 1)
        a1 = (a0 + 1) % A
        fu = (u - a0.astype(dtype)).astype(dtype)
        b0 = np.floor(v).astype(np.int64)
        b1 = np.minimum(b0 + 1, N - 1)
        fv = (v - b0.astype(dtype)).astype(dtype)
        one = ft(1.0)
        p0 = (one - fu) * z(b0, a0) + fu * z(b0, a1)
        p1 = (one - fu) * z(b1, a0) + fu * z(b1, a1)
        out = np.rint((one - fv) * p0 + fv * p1)
    return np.clip(np.where(outside, 0, out), 0, 255).astype(np.uint8)


def pose_apply(pose, xyz):
    """map-frame positions of sensor-frame points under pose (qx qy qz qw tx ty tz), float64 (for the closed-loop checks)"""
    p = np.asarray(pose, np.float64)
    q = np.broadcast_to(p[:4], (len(xyz), 4))
    return q_rot(q, np.asarray(xyz, np.float64)) + p[4:]


__all__ = ["q_mul", "q_conj", "q_rot", "v_dot", "sweep_table", "compensate_points", "cartesian_sweep", "pose_apply", "POINT_DTYPE"]


# ---- the inputs of the Cartesian comparison (tests/test_gpu_deskew.py), kept here so that tests/test_deskew_host.py can hold the
# same inputs to the float64 form of the restatement
# (theta_min off zero: with azimuth 0 along a pixel axis and an odd n_angles, the pixels straight behind the sensor sit at u = n_angles / 2
# exactly, a tie of rintf that float32 and float64 break differently)
CART_N_CELLS, CART_SCROLL, CART_GAIN, CART_THETA_MIN = 96, 5, 0.05, 0.1


def cart_case(n_frames, n_angles, bilinear, resolution):
    """-> (images u8 [n][96][n_angles], per-azimuth poses [n][n_angles][7], reference poses [n][7], sensor velocities [n][3]).
    Bilinear frames are noise (every rounding of the interpolation shows); nearest frames are a ramp whose neighbouring cells differ
    by one grey level, in range and across the azimuth wrap, so that a pixel whose rintf sits on a rounding boundary stays within the
    criterion while any systematic error of a cell moves every pixel.  The sweeps: 4 m/s and more forward, a yaw rate, 0.25 s, the
    reference azimuth different in every frame: about 1 m (a sixth of the image's range) of motion and 0.2 m of Doppler shift."""
    from radarays_ros_amd import scenes
    rs = np.random.RandomState(100 * n_angles + 10 * n_frames + int(bilinear))
    if bilinear:
        imgs = rs.randint(0, 256, (n_frames, CART_N_CELLS, n_angles)).astype(np.uint8)
    else:
        col = np.arange(n_angles)
        tri = np.minimum(col, n_angles - col)
        imgs = np.stack([(np.arange(CART_N_CELLS)[:, None] + tri[None, :] + 7 * f) for f in range(n_frames)]).astype(np.uint8)
    az, ref, vel = [], [], []
    for f in range(n_frames):
        pose = scenes.yaw_pose(0.3 * f, -0.2 * f, 0.1, 0.4 + 0.5 * f)
        twist = [4.0 + f, 0.3 * f, 0.0, 0.0, 0.0, 0.5 - 0.4 * f]
        p, v = scenes.sweep_poses(pose, twist, 0.25, n_angles, ref_azimuth=(n_angles // 2 + 9 * f) % n_angles)
        az.append(p); ref.append(pose); vel.append(v)
    return imgs, np.stack(az), np.stack(ref).astype(np.float32), np.stack(vel)


def cart_pixel_size(width, resolution):
    return 2 * CART_N_CELLS * resolution / width          # the image reaches a little past the last bin


CART_CASES = [(n_frames, n_angles, width, bilinear, iterations)
              for n_frames in (1, 3) for n_angles in (37, 64) for width in (33, 64) for bilinear in (False, True) for iterations in (1, 2, 3)]
