"""Sweep compensation on the GPU (rr_deskew.hip) against the numpy restatement of its definitions (tests/deskew_ref.py): the
record table and the compensated points bit for bit (the Doppler term to the ulps of cosf / sinf), the compensated Cartesian
image exact up to the ulps of atan2f, byte for byte the plain conversion under an identity table; and closed loops through the
simulation: a wall seen from a moving sensor, with and without the Doppler shift, lands where the standing sensor sees it."""
import ctypes as C

import numpy as np
import pytest

import deskew_ref as R
from common import golden_beams
from radarays_ros_amd import native, params, scenes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
N_CELLS = 96


def conv_ctx(n_angles, scroll=0, n_cells=N_CELLS, theta_min=0.0):
    """a context with a config and no mesh: what a caller converting real images has"""
    c = native.Context(0)
    c.set_config(params.kaist_preset(n_cells=n_cells, scroll_image=scroll), n_angles, theta_min=theta_min)
    return c


def geometry(ctx):
    g = ctx._rrcfg
    return dict(scroll=g.scroll_image, theta_min=g.theta_min, theta_inc=g.theta_inc, resolution=g.resolution)


def random_poses(rs, shape):
    q = rs.standard_normal(shape + (4,))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    return np.concatenate([q, rs.uniform(-5, 5, shape + (3,))], -1).astype(np.float32)


def random_table(rs, n, n_angles, dr=0.3):
    """small rigid motions and range shifts per azimuth: SWEEP_DTYPE [n][n_angles]"""
    t = native.identity_sweep_table(n, n_angles)
    q = np.concatenate([rs.uniform(-0.1, 0.1, (n, n_angles, 3)), np.ones((n, n_angles, 1))], -1)
    t["q"] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    t["t"] = rs.uniform(-1, 1, (n, n_angles, 3))
    t["dr"] = rs.uniform(-dr, dr, (n, n_angles))
    return t


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)


def back(t, dtype, shape):
    return t.cpu().numpy().view(dtype).reshape(shape)


def same_points(got, want):
    for k in ("column", "bin", "intensity"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("x", "y", "z"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)) or \
            (np.array_equal(np.isnan(got[k]), np.isnan(want[k])) and np.array_equal(got[k][~np.isnan(got[k])], want[k][~np.isnan(want[k])])), k


# ---- 1. the table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gain", [0.0, 0.05])
@pytest.mark.parametrize("n_frames,n_angles", [(1, 37), (3, 37), (1, 64), (3, 64)])
def test_table_matches_the_restatement(n_frames, n_angles, gain):
    ctx = conv_ctx(n_angles, theta_min=0.2)
    rs = np.random.RandomState(n_frames * 100 + n_angles)
    az, ref = random_poses(rs, (n_frames, n_angles)), random_poses(rs, (n_frames,))
    vel = rs.uniform(-20, 20, (n_frames, 3)).astype(np.float32)
    got = ctx.sweep_table(az, ref, vel, gain)
    g = geometry(ctx)
    want = R.sweep_table(az, ref, vel, gain, g["theta_min"], g["theta_inc"])
    assert got["q"].tobytes() == want["q"].tobytes() and got["t"].tobytes() == want["t"].tobytes()
    if gain == 0.0:
        assert np.all(got["dr"].view(np.uint32) == 0)                  # +0 exactly
    else:
        # dr = gain * (v_s . u) with u a unit vector whose components carry the ulps of cosf / sinf: the detector test's bound for
        # r * cosf (1e-6 * r + 1e-6, tests/test_gpu_detect.py) at r = 1, scaled by |gain| * |v_s|
        bound = (1e-6 * 1.0 + 1e-6) * abs(gain) * np.linalg.norm(vel.astype(np.float64), axis=1)[:, None]
        assert np.all(np.abs(got["dr"].astype(np.float64) - want["dr"]) <= bound)
        assert np.abs(want["dr"]).max() > 0.1
    # without velocities the shift is zero whatever the gain; the device form gives the same bytes as the host form
    assert np.all(ctx.sweep_table(az, ref, None, 0.05)["dr"].view(np.uint32) == 0)
    d_az, d_ref, d_vel = dev(az), dev(ref), dev(vel)
    d_tab = torch.zeros(n_frames * n_angles * 32, dtype=torch.uint8, device=DEV)
    ctx.sweep_table_device(d_az.data_ptr(), d_ref.data_ptr(), n_frames, d_tab.data_ptr(), d_vel.data_ptr(), gain)
    ctx.synchronize()
    assert back(d_tab, native.SWEEP_DTYPE, (n_frames, n_angles)).tobytes() == got.tobytes()


def test_host_table_refuses_what_it_can_see():
    ctx = conv_ctx(16)
    L, h = ctx._L, ctx._h
    ident = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
    az, ref, vel = np.tile(ident, (2, 16, 1)), np.tile(ident, (2, 1)), np.ones((2, 3), np.float32)
    table = np.full(2 * 16 * 8, 0x5A5A5A5A, np.uint32)

    def call(a, r, v, gain, n=2):
        return L.rr_sweep_table(h, a.ctypes.data, r.ctypes.data, None if v is None else v.ctypes.data, gain, n, table.ctypes.data)

    bad_az, bad_q, off_q, bad_ref, bad_vel = az.copy(), az.copy(), az.copy(), ref.copy(), vel.copy()
    bad_az[1, 3, 5] = np.inf; bad_q[0, 0, 3] = np.nan; off_q[1, 15, 3] = 1.001; bad_ref[1, :4] = (0, 0, 0, 0.99); bad_vel[0, 2] = np.nan
    for args in ((bad_az, ref, None, 0.0), (bad_q, ref, None, 0.0), (off_q, ref, None, 0.0), (az, bad_ref, None, 0.0), (az, ref, bad_vel, 0.1),
                 (az, ref, vel, float("nan")), (az, ref, vel, float("inf"))):
        assert call(*args) == -3
    assert call(az, ref, vel, 0.1, n=0) == -3 and call(az, ref, vel, 0.1, n=65536) == -3
    assert b"rr_sweep_table" in L.rr_last_error(h)
    assert np.all(table == 0x5A5A5A5A)
    ok_q = az.copy(); ok_q[1, 15, 3] = 1.0004                           # squared norm 1.0008: inside the 1e-3
    assert call(ok_q, ref, vel, 0.1) == 0 and not np.any(table == 0x5A5A5A5A)


# ---- 2. the points -----------------------------------------------------------------------------------------------------
DETECTORS = [dict(method=0, guard_cells=2, train_cells=16, k=12, min_intensity=1, min_bin=0, cfar_scale=3.0),
             dict(method=1, guard_cells=2, train_cells=16, k=12, min_intensity=1, min_bin=0, cfar_scale=3.0)]


def noisy_images(n, n_angles, seed):
    rs = np.random.RandomState(seed)
    imgs = rs.randint(0, 30, (n, N_CELLS, n_angles)).astype(np.uint8)
    peaks = rs.rand(n, N_CELLS, n_angles) < 0.10
    imgs[peaks] = rs.randint(80, 256, int(peaks.sum()))
    imgs[:, 0, ::3] = 240                                               # detections in bin 0 too
    return imgs


@pytest.mark.parametrize("det", DETECTORS, ids=["cfar", "k12"])
@pytest.mark.parametrize("n_angles", [37, 64])
def test_points_match_the_restatement(n_angles, det):
    n, scroll = 3, 7
    ctx = conv_ctx(n_angles, scroll)
    g = geometry(ctx)
    imgs = noisy_images(n, n_angles, seed=n_angles)
    d_imgs = dev(imgs)
    offs = torch.zeros((n, n_angles + 1), dtype=torch.int32, device=DEV)
    ctx.detect_device(d_imgs.data_ptr(), n, det, None, 0, offs.data_ptr())
    ctx.synchronize()
    totals = offs.cpu().numpy().view(np.uint32)[:, -1]
    mp = int(totals.max())
    assert totals.min() > 256                                           # more than one workgroup of points per frame
    pts = torch.zeros(n * mp * 24, dtype=torch.uint8, device=DEV)
    ctx.detect_device(d_imgs.data_ptr(), n, det, pts.data_ptr(), mp, offs.data_ptr())
    rs = np.random.RandomState(5)
    az, ref = random_poses(rs, (n, n_angles)), random_poses(rs, (n,))
    vel = rs.uniform(-20, 20, (n, 3)).astype(np.float32)
    table = ctx.sweep_table(az, ref, vel, 0.05)                         # the GPU's own table: only the point kernel is under test
    table["dr"][1] = 0.0
    table["dr"][1, ::2] = 0.5 * g["resolution"] + 0.01                  # frame 1: bin 0 (r = half a bin) of every other azimuth has rc < 0
    table["dr"][2, 3] = np.inf; table["dr"][2, 4] = np.nan
    d_tab = dev(table)
    canary = 0xA5
    out = torch.full((n * mp * 24 + 4096,), canary, dtype=torch.uint8, device=DEV)
    ctx.compensate_points_device(pts.data_ptr(), offs.data_ptr(), n, mp, d_tab.data_ptr(), out.data_ptr())
    ctx.synchronize()
    h_in = back(pts, native.POINT_DTYPE, (n, mp))
    h_out = out.cpu().numpy()
    assert np.all(h_out[n * mp * 24:] == canary)
    got = h_out[:n * mp * 24].view(native.POINT_DTYPE).reshape(n, mp)
    n_nan = 0
    for f in range(n):
        m = int(totals[f])
        want = R.compensate_points(h_in[f, :m], table[f], g["scroll"], g["resolution"])
        same_points(got[f, :m], want)
        assert np.all(got[f, m:].view(np.uint8) == canary)              # slots beyond the count are not touched
        n_nan += int(np.isnan(want["x"]).sum())
        if f == 1:
            lost = (h_in[f, :m]["bin"] == 0) & (((h_in[f, :m]["column"].astype(int) - scroll) % n_angles) % 2 == 0)
            assert lost.any() and np.all(np.isnan(got[f, :m]["x"][lost])) and not np.any(np.isnan(got[f, :m]["x"][~lost]))
    assert n_nan > 0
    # in place: the same bytes
    ctx.compensate_points_device(pts.data_ptr(), offs.data_ptr(), n, mp, d_tab.data_ptr(), None)
    ctx.synchronize()
    h_inplace = back(pts, native.POINT_DTYPE, (n, mp))
    for f in range(n):
        m = int(totals[f])
        assert h_inplace[f, :m].tobytes() == got[f, :m].tobytes() and h_inplace[f, m:].tobytes() == h_in[f, m:].tobytes()
    # the host form
    host = ctx.compensate_points([h_in[f, :int(totals[f])] for f in range(n)], offs.cpu().numpy().view(np.uint32), table)
    for f in range(n):
        assert host[f].tobytes() == got[f, :int(totals[f])].tobytes()


def test_truncated_points_leave_the_canary():
    n_angles, n = 64, 2
    ctx = conv_ctx(n_angles, 3)
    imgs = noisy_images(n, n_angles, seed=1)
    d_imgs = dev(imgs)
    det = DETECTORS[0]
    mp = 100
    offs = torch.zeros((n, n_angles + 1), dtype=torch.int32, device=DEV)
    pts = torch.zeros(n * mp * 24, dtype=torch.uint8, device=DEV)
    ctx.detect_device(d_imgs.data_ptr(), n, det, pts.data_ptr(), mp, offs.data_ptr())
    table = random_table(np.random.RandomState(2), n, n_angles)
    d_tab = dev(table)
    out = torch.full((n * mp * 24 + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    ctx.compensate_points_device(pts.data_ptr(), offs.data_ptr(), n, mp, d_tab.data_ptr(), out.data_ptr())
    ctx.synchronize()
    assert np.all(offs.cpu().numpy().view(np.uint32)[:, -1] > mp)       # every frame is truncated
    h = out.cpu().numpy()
    assert np.all(h[n * mp * 24:] == 0xA5)
    got, h_in, g = h[:n * mp * 24].view(native.POINT_DTYPE).reshape(n, mp), back(pts, native.POINT_DTYPE, (n, mp)), geometry(ctx)
    for f in range(n):
        same_points(got[f], R.compensate_points(h_in[f], table[f], g["scroll"], g["resolution"]))


# ---- 3. identity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_angles", [37, 64])
@pytest.mark.parametrize("bilinear", [False, True], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("width", [33, 64])
def test_identity_table_reproduces_the_plain_conversion(width, bilinear, n_angles):
    n = 3
    ctx = conv_ctx(n_angles, 5)
    imgs = np.random.RandomState(width + n_angles).randint(0, 256, (n, N_CELLS, n_angles)).astype(np.uint8)
    ps = 2 * N_CELLS * ctx._rrcfg.resolution / width
    want = ctx.polar_to_cartesian(imgs, width, ps, bilinear)
    ident = native.identity_sweep_table(n, n_angles)
    for it in (1, 3):
        got = ctx.polar_to_cartesian_sweep(imgs, ident, width, ps, bilinear, it)
        assert got.tobytes() == want.tobytes(), it
    assert want.any()


@pytest.mark.parametrize("n_angles", [5, 64])
@pytest.mark.parametrize("width", [2, 33])
def test_the_three_resamplers_agree_off_the_default_geometry(width, n_angles):
    """the plain, the identity-sweep and the label resampler share one geometry (rr_polar.h); held here where the identity test above and
    tests/test_gpu_notes.py's labels against the u8 resampler do not look: theta_min off zero, a counter-clockwise sweep, the last scroll,
    five azimuths, 37 cells, a 2 x 2 image.  At width 2 the four pixels lie at one range: the second pixel size puts them beyond the last bin"""
    n, n_cells = 2, 37
    ctx = native.Context(0)
    ctx.set_config(params.kaist_preset(n_cells=n_cells, scroll_image=n_angles - 1), n_angles, theta_min=0.7, theta_inc=2 * np.pi / n_angles)
    g = ctx._rrcfg
    assert g.theta_inc > 0 and g.scroll_image == n_angles - 1 and abs(g.theta_min - 0.7) < 1e-6
    u8 = np.random.RandomState(width + n_angles).randint(1, 256, (n, n_cells, n_angles)).astype(np.uint8)      # no zero: 0 is beyond range
    ident = native.identity_sweep_table(n, n_angles)
    seen = []
    for reach in (2.2, 3.2):                                            # the corners, then at width 2 every pixel, beyond the last bin
        ps = reach * n_cells * g.resolution / width
        near = ctx.polar_to_cartesian(u8, width, ps, False)
        lab = ctx.polar_to_cartesian_labels(u8.astype(np.uint32), width, ps)
        beyond = lab == native.LABEL_NONE
        assert np.array_equal(np.where(beyond, 0, lab), near.astype(np.uint32)) and np.array_equal(beyond, near == 0)
        bil = ctx.polar_to_cartesian(u8, width, ps, True)
        for it in (1, 3):
            assert ctx.polar_to_cartesian_sweep(u8, ident, width, ps, False, it).tobytes() == near.tobytes(), (reach, it)
            assert ctx.polar_to_cartesian_sweep(u8, ident, width, ps, True, it).tobytes() == bil.tobytes(), (reach, it)
        seen.append(beyond)
    assert any(b.any() for b in seen) and not all(b.all() for b in seen)


# ---- 4. a real table ---------------------------------------------------------------------------------------------------
_cart = {}


def cart_inputs(n_frames, n_angles, bilinear):
    """the inputs, the GPU's table and the context of one group of cases, made once"""
    key = (n_frames, n_angles, bilinear)
    if key not in _cart:
        ctx = conv_ctx(n_angles, R.CART_SCROLL, theta_min=R.CART_THETA_MIN)
        imgs, az, ref, vel = R.cart_case(n_frames, n_angles, bilinear, ctx._rrcfg.resolution)
        _cart[key] = (ctx, imgs, ctx.sweep_table(az, ref, vel, R.CART_GAIN))
    return _cart[key]


@pytest.mark.parametrize("n_frames,n_angles,width,bilinear,iterations", R.CART_CASES)
def test_cartesian_matches_the_restatement(n_frames, n_angles, width, bilinear, iterations):
    ctx, imgs, table = cart_inputs(n_frames, n_angles, bilinear)
    g = geometry(ctx)
    ps = R.cart_pixel_size(width, g["resolution"])
    got = ctx.polar_to_cartesian_sweep(imgs, table, width, ps, bilinear, iterations)
    plain = ctx.polar_to_cartesian(imgs, width, ps, bilinear)
    for f in range(n_frames):
        want = R.cartesian_sweep(imgs[f], table[f], width, ps, bilinear, iterations, **g)
        d = np.abs(got[f].astype(int) - want)
        print("frame %d: max |diff| %d, share %.2e" % (f, d.max(), np.mean(d > 0)))
        assert d.max() <= 1 and np.mean(d > 0) <= 1e-3, (d.max(), np.mean(d > 0))
        assert np.mean(got[f] != plain[f]) > 0.3                       # the table moves most pixels: the comparison has power


# ---- 5. closed loop ----------------------------------------------------------------------------------------------------
# One wall, 16 m wide and 10 m tall, 12 m ahead of the reference pose (the map's x = 12 plane), seen by a sensor that drives at it.
# theta_min = pi: azimuth 0 looks backwards, the wall is seen around azimuth 32, in the middle of the sweep, away from the seam.
WALL_X, A_LOOP, CELLS_LOOP, SPEED, SWEEP_TIME, GAIN = 12.0, 64, 320, 20.0, 0.1, 0.05
REF_POSE = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
TWIST = [SPEED, 0.0, 0.0, 0.0, 0.0, 1.0]


def wall_ctx():
    verts = np.array([[WALL_X, -8, -5], [WALL_X, 8, -5], [WALL_X, 8, 5], [WALL_X, -8, 5]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    cfg = params.kaist_preset(n_reflections=1, n_samples=50, ambient_noise=0, signal_denoising=0, n_cells=CELLS_LOOP)
    ctx = native.Context(0)
    ctx.set_mesh(verts, faces, np.zeros(2, np.uint32))
    ctx.set_materials(params.kaist_materials(), [1], 0)
    ctx.set_config(cfg, A_LOOP, theta_min=np.pi)
    ctx.set_beam_samples(golden_beams(50))
    return ctx, cfg


def plane_error(points, pose):
    xyz = np.stack([points["x"], points["y"], points["z"]], -1)
    return np.abs(R.pose_apply(pose, xyz)[:, 0] - WALL_X)


def wall_row(cart):
    """the row of the wall's brightest response along the centre column (the middle of its plateau)"""
    col = cart[:, cart.shape[1] // 2].astype(int)
    return float(np.mean(np.nonzero(col == col.max())[0]))


@pytest.mark.parametrize("case", ["motion_and_doppler", "motion_only", "doppler_only"])
def test_closed_loop_a_wall_lands_where_the_standing_sensor_sees_it(case):
    ctx, cfg = wall_ctx()
    res = cfg.resolution
    gain = 0.0 if case == "motion_only" else GAIN
    twist = [0.0] * 6 if case == "doppler_only" else TWIST
    poses, vel = scenes.sweep_poses(REF_POSE, twist, SWEEP_TIME, A_LOOP, 0)
    if case == "doppler_only":
        vel = np.array([SPEED, 0, 0], np.float32)                       # an identity motion table, the velocity alone
    # the conditions on the inputs, from the numbers chosen: the sweep's displacement is at least 20 bins, the Doppler shift of a
    # head-on echo at least 10; the wall's azimuths (26..38 of 64, sweep start = reference) are measured 0.81 m and more ahead
    assert SPEED * SWEEP_TIME >= 20 * res and GAIN * SPEED >= 10 * res
    assert SPEED * SWEEP_TIME * 26 / 64 > 5 * res and GAIN * SPEED * np.cos(np.arctan2(8, WALL_X - SPEED * SWEEP_TIME)) > 5 * res
    det = dict(method=1, k=1, min_intensity=1)
    # run A: the standing sensor
    img_a = ctx.simulate(REF_POSE)[0]
    pts_a, _ = ctx.detect(img_a, det)
    # run B: the moving sensor
    ctx.set_motion_poses(poses)
    img_b = ctx.simulate_doppler(REF_POSE, sensor_vel=vel, gain=gain, echo_stride=0, want_vel_img=False)[0] if gain else ctx.simulate(REF_POSE)[0]
    ctx.set_motion_poses(None)
    pts_b, offs_b = ctx.detect(img_b, det)
    table = ctx.sweep_table(poses, REF_POSE, vel if gain else None, gain)
    comp = ctx.compensate_points(pts_b, offs_b, table)[0]
    lit = np.intersect1d(pts_a[0]["column"], pts_b[0]["column"])        # the lit columns of both runs
    assert len(lit) >= 8
    a, b, c = (p[np.isin(p["column"], lit)] for p in (pts_a[0], pts_b[0], comp))
    err_a, err_raw, err_comp = (np.median(plane_error(p, REF_POSE)) for p in (a, b, c))
    print("%s: median |distance to the wall| A %.4f m, B raw %.4f m, B compensated %.4f m (bin %.4f m)" % (case, err_a, err_raw, err_comp, res))
    assert err_raw > 5 * res                                            # without compensation the wall is bent away: the test has power
    assert err_comp <= err_a + res                                      # one bin: the Doppler chain rounds the shifted cell to an integer
    # The bird's-eye images, one pixel per bin, 513 wide (+-15.2 m): the compensated image of B against the plain image of A.  The
    # centre column is the map's x axis; the wall's response there comes from azimuth 32.  Bound: B's shifted cell is an integer bin
    # (at most 1 bin = 1 pixel from where A's cell lies), and each image places a bin's response at the pixel nearest to its
    # centre (at most 1 pixel between the two resamplings, whose sensor positions differ by a fraction of a pixel): 1 pixel + 1 bin
    # = 2 pixels at this pixel size.
    width, ps = 513, res
    cart_a = ctx.polar_to_cartesian(img_a, width, ps, False)[0]
    cart_raw = ctx.polar_to_cartesian(img_b, width, ps, False)[0]
    cart_b = ctx.polar_to_cartesian_sweep(img_b, table, width, ps, False, 2)[0]
    rows = wall_row(cart_a), wall_row(cart_raw), wall_row(cart_b)
    print("%s: wall row along the centre column: A %.1f, B raw %.1f, B compensated %.1f" % ((case,) + rows))
    assert abs(rows[0] - (256 - WALL_X / ps)) <= 2                      # A sees the wall at 12 m
    assert abs(rows[1] - rows[0]) > 5
    assert abs(rows[2] - rows[0]) <= 1 + res / ps


# ---- 6. two streams ----------------------------------------------------------------------------------------------------
def test_two_streams_compensate_different_batches_at_once():
    n, n_angles, mp, width = 8, 64, 64 * 12, 64
    ctx = conv_ctx(n_angles, 11)
    g = geometry(ctx)
    det = DETECTORS[1]
    ps = 2 * N_CELLS * g["resolution"] / width
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    work = []
    for seed, s in ((21, s1), (22, s2)):
        rs = np.random.RandomState(seed)
        imgs = noisy_images(n, n_angles, seed)
        az, ref = random_poses(rs, (n, n_angles)), random_poses(rs, (n,))
        vel = rs.uniform(-20, 20, (n, 3)).astype(np.float32)
        bufs = dict(imgs=dev(imgs), az=dev(az), ref=dev(ref), vel=dev(vel),
                    pts=torch.zeros(n * mp * 24, dtype=torch.uint8, device=DEV), offs=torch.zeros((n, n_angles + 1), dtype=torch.int32, device=DEV),
                    tab=torch.zeros(n * n_angles * 32, dtype=torch.uint8, device=DEV), tab2=dev(random_table(rs, n, n_angles)),
                    cart=torch.zeros((n, width, width), dtype=torch.uint8, device=DEV))
        work.append((bufs, s))
    torch.cuda.synchronize()

    def enqueue(b, stream):
        p = {k: v.data_ptr() for k, v in b.items()}
        ctx.sweep_table_device(p["az"], p["ref"], n, p["tab"], p["vel"], 0.05, stream)
        ctx.detect_device(p["imgs"], n, det, p["pts"], mp, p["offs"], stream)
        ctx.compensate_points_device(p["pts"], p["offs"], n, mp, p["tab"], None, stream)
        ctx.polar_to_cartesian_sweep_device(p["imgs"], n, width, ps, p["tab2"], p["cart"], True, 2, stream)

    def results(b):
        return tuple(b[k].cpu().numpy().tobytes() for k in ("tab", "pts", "cart"))

    for b, s in work:
        enqueue(b, s.cuda_stream)
    torch.cuda.synchronize()
    together = [results(b) for b, _ in work]
    for b, _ in work:                                                   # one after the other, on the context's stream
        b["pts"].zero_(); b["tab"].zero_(); b["cart"].zero_()
        torch.cuda.synchronize()
        enqueue(b, None)
        ctx.synchronize()
    assert [results(b) for b, _ in work] == together
    assert together[0] != together[1] and any(together[0][2])


# ---- 7. the frame path -------------------------------------------------------------------------------------------------
def test_compensation_leaves_the_frame_path_alone():
    s = scenes.box12()
    cfg = params.kaist_preset(n_reflections=2, ambient_noise=0)
    ctx = native.Context(0)
    ctx.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    ctx.set_materials(params.kaist_materials(), s["object_materials"], 0)
    ctx.set_config(cfg)
    ctx.set_beam_samples(golden_beams(100))
    pose = scenes.default_pose("box12")
    before, f_before, _ = ctx.simulate(pose, want_f32=True)
    poses, vel = scenes.sweep_poses(pose, [5.0, 0, 0, 0, 0, 0.5], 0.25, 400, 200)
    table = ctx.sweep_table(poses, pose, vel, 0.05)
    pts, offs = ctx.detect(before, method=1, k=4)
    ctx.compensate_points(pts, offs, table)
    ctx.polar_to_cartesian_sweep(before, table, 200, 0.1, True, 3)
    ctx.polar_to_cartesian_sweep(before, table, 99, 0.2, False, 1)
    after, f_after, _ = ctx.simulate(pose, want_f32=True)
    assert np.array_equal(before, after) and np.array_equal(f_before, f_after)
    assert before.any()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------
def test_refusals_return_minus_3_and_write_nothing():
    n_angles, n = 16, 2
    ctx = conv_ctx(n_angles, n_cells=64)
    L, h = ctx._L, ctx._h
    canary = 0x5A
    imgs = dev(np.zeros((n, 64, n_angles), np.uint8))
    fill = lambda size: torch.full((size,), canary, dtype=torch.uint8, device=DEV)   # noqa: E731
    az, ref, vel = fill(n * n_angles * 28), fill(n * 28), fill(n * 12)
    tab, pts, out, cart = fill(n * n_angles * 32 + 16), fill(n * 32 * 24), fill(n * 32 * 24), fill(n * 16 * 16)
    offs = torch.zeros((n, n_angles + 1), dtype=torch.int32, device=DEV)
    offs[:, -1] = 32

    def ccfg(width=16, interpolation=1, pixel_size=0.5):
        c = native.RRCartesianConfig()
        c.width, c.interpolation, c.pixel_size = width, interpolation, pixel_size
        return c

    P = lambda t: t.data_ptr()   # noqa: E731
    good = ccfg()
    # the table
    for args in ((None, P(ref), P(vel), 0.1, n, P(tab)), (P(az), None, P(vel), 0.1, n, P(tab)), (P(az), P(ref), P(vel), 0.1, n, None),
                 (P(az), P(ref), P(vel), 0.1, 0, P(tab)), (P(az), P(ref), P(vel), 0.1, 65536, P(tab)), (P(az), P(ref), P(vel), float("nan"), n, P(tab)),
                 (P(az), P(ref), P(vel), float("inf"), n, P(tab)), (P(az), P(ref), P(vel), 0.1, n, P(tab) + 4)):
        assert L.rr_sweep_table_device(h, *args, None) == -3
    assert b"rr_sweep_table_device" in L.rr_last_error(h)
    # the points
    for args in ((None, P(offs), n, 32, P(tab), P(out)), (P(pts), None, n, 32, P(tab), P(out)), (P(pts), P(offs), n, 32, None, P(out)),
                 (P(pts), P(offs), n, 32, P(tab), None), (P(pts), P(offs), 0, 32, P(tab), P(out)), (P(pts), P(offs), 65536, 32, P(tab), P(out)),
                 (P(pts), P(offs), n, -1, P(tab), P(out)), (P(pts), P(offs), n, 32, P(tab) + 8, P(out))):
        assert L.rr_compensate_points_device(h, *args, None) == -3
    # the image
    for c, it in ((good, 0), (good, 9), (good, -1), (ccfg(width=0), 2), (ccfg(width=8193), 2), (ccfg(interpolation=2), 2), (ccfg(pixel_size=0.0), 2),
                  (ccfg(pixel_size=float("nan")), 2)):
        assert L.rr_polar_to_cartesian_sweep_device(h, P(imgs), n, C.byref(c), P(tab), it, P(cart), None) == -3
    for args in ((None, n, C.byref(good), P(tab), 2, P(cart)), (P(imgs), n, None, P(tab), 2, P(cart)), (P(imgs), n, C.byref(good), None, 2, P(cart)),
                 (P(imgs), n, C.byref(good), P(tab), 2, None), (P(imgs), 0, C.byref(good), P(tab), 2, P(cart)),
                 (P(imgs), n, C.byref(good), P(tab) + 4, 2, P(cart))):
        assert L.rr_polar_to_cartesian_sweep_device(h, *args, None) == -3
    # more azimuths than a workgroup's LDS holds records of: refused by the image call alone
    wide = conv_ctx(2049, n_cells=4)
    w_imgs, w_tab, w_cart = dev(np.zeros((1, 4, 2049), np.uint8)), fill(2049 * 32), fill(16 * 16)
    assert wide._L.rr_polar_to_cartesian_sweep_device(wide._h, P(w_imgs), 1, C.byref(good), P(w_tab), 2, P(w_cart), None) == -3
    assert b"65536" in wide._L.rr_last_error(wide._h)
    # host forms: the canaries are host arrays
    h_tab = np.full(n * n_angles * 8, 0x5A5A5A5A, np.uint32)
    h_pts, h_out, h_cart = np.full(n * 32 * 24, canary, np.uint8), np.full(n * 32 * 24, canary, np.uint8), np.full(n * 16 * 16, canary, np.uint8)
    h_offs, h_imgs = offs.cpu().numpy(), np.zeros((n, 64, n_angles), np.uint8)
    ident = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float32), (n, n_angles, 1))
    assert L.rr_sweep_table(h, ident.ctypes.data, ident.ctypes.data, None, 0.0, 0, h_tab.ctypes.data) == -3
    assert L.rr_sweep_table(h, ident.ctypes.data, None, None, 0.0, n, h_tab.ctypes.data) == -3
    assert L.rr_compensate_points(h, h_pts.ctypes.data, h_offs.ctypes.data, n, -1, h_tab.ctypes.data, h_out.ctypes.data) == -3
    assert L.rr_compensate_points(h, h_pts.ctypes.data, h_offs.ctypes.data, n, 32, None, h_out.ctypes.data) == -3
    assert L.rr_polar_to_cartesian_sweep(h, h_imgs.ctypes.data, n, C.byref(good), h_tab.ctypes.data, 0, h_cart.ctypes.data) == -3
    assert L.rr_polar_to_cartesian_sweep(h, h_imgs.ctypes.data, n, C.byref(ccfg(width=0)), h_tab.ctypes.data, 2, h_cart.ctypes.data) == -3
    torch.cuda.synchronize()
    assert np.all(h_tab == 0x5A5A5A5A) and np.all(h_out == canary) and np.all(h_cart == canary)
    for t in (tab, out, cart, w_cart, pts):
        assert bool((t == canary).all())
    # without a config: -2
    bare = native.Context(0)
    assert bare._L.rr_sweep_table_device(bare._h, P(az), P(ref), P(vel), 0.1, n, P(tab), None) == -2
    assert bare._L.rr_compensate_points_device(bare._h, P(pts), P(offs), n, 32, P(tab), P(out), None) == -2
    assert bare._L.rr_polar_to_cartesian_sweep_device(bare._h, P(imgs), n, C.byref(good), P(tab), 2, P(cart), None) == -2
    torch.cuda.synchronize()
    for t in (tab, out, cart):
        assert bool((t == canary).all())


# ---- 9. the facade -----------------------------------------------------------------------------------------------------
def test_radar_facade_simulate_sweep():
    from radarays_ros_amd import radar
    s = scenes.box12()
    r = radar.RadarHIP(s["verts"], s["faces"], s["face_object_id"])
    r.loadParams(params.kaist_materials(), s["object_materials"], 0)
    r.updateDynCfg(params.kaist_preset(n_reflections=2, ambient_noise=0, n_cells=512))
    r.setBeamSamples(golden_beams(100))
    pose = scenes.default_pose("box12")
    twist, T, gain = [3.0, 0.5, 0.0, 0.0, 0.0, 0.8], 0.25, 0.02
    r.updateTsm(pose)
    assert r.simulate() is not None                                     # (pushes the config)
    ctx = r.context
    before = {"image": ctx.simulate(pose)[0]}                           # no motion table installed: a plain frame
    out = r.simulate_sweep(pose, twist, T, gain=gain, detect=dict(method=1, k=3), cartesian=dict(width=65, pixel_size=0.4, bilinear=False, iterations=3))
    poses, vel = scenes.sweep_poses(pose, twist, T, 400, 0)
    assert np.array_equal(out["poses"], poses) and np.array_equal(out["sensor_vel"], vel)
    ctx.set_motion_poses(poses)
    img = ctx.simulate_doppler(pose, sensor_vel=vel, gain=gain, echo_stride=0, want_vel_img=False)[0]
    ctx.set_motion_poses(None)
    table = ctx.sweep_table(poses, pose, vel, gain)
    pts, offs = ctx.detect(img, method=1, k=3)
    assert np.array_equal(out["image"], img) and out["table"].tobytes() == table[0].tobytes()
    assert out["points_raw"].tobytes() == pts[0].tobytes() and np.array_equal(out["offsets"], offs[0])
    assert out["points"].tobytes() == ctx.compensate_points(pts, offs, table)[0].tobytes() and len(out["points"]) > 0
    assert np.array_equal(out["cartesian_raw"], ctx.polar_to_cartesian(img, 65, 0.4, False)[0])
    assert np.array_equal(out["cartesian"], ctx.polar_to_cartesian_sweep(img, table, 65, 0.4, False, 3)[0])
    assert not np.array_equal(out["cartesian"], out["cartesian_raw"]) and not np.array_equal(out["image"], before["image"])
    # the motion table is left as it was found: none here ...
    assert np.array_equal(ctx.simulate(pose)[0], before["image"])
    # ... and the caller's own, also when an inner call raises
    mine = np.tile(scenes.yaw_pose(1.0, 1.5, 0.2, -0.4), (400, 1))
    r.setMotionPoses(mine)
    with_mine = ctx.simulate(pose)[0]
    assert not np.array_equal(with_mine, before["image"])
    with pytest.raises(ValueError):
        r.simulate_sweep(pose, twist, T, cartesian=dict(width=0, pixel_size=0.4))
    assert np.array_equal(ctx.simulate(pose)[0], with_mine)
    r.simulate_sweep(pose, twist, T, gain=gain)
    assert np.array_equal(ctx.simulate(pose)[0], with_mine)
