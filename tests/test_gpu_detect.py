"""Point clouds and Cartesian images on the GPU (rr_detect.hip) against the numpy restatement of their definitions
(tests/detect_ref.py): detections, order and offsets bit for bit, xyz to f32 trigonometry ulps; Cartesian pixels exact up to
the ulps of atan2f / sqrtf.  Plus the simulation's frame convention, truncation, refusals, and isolation from the frame
path."""
import ctypes as C

import numpy as np
import pytest

import detect_ref as R
from common import golden_beams, materials_for
from radarays_ros_amd import native, params, scenes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"


def config(n_cells, scroll=0, **kw):
    return params.kaist_preset(n_cells=n_cells, scroll_image=scroll, **kw)


def conv_ctx(n_cells, n_angles=400, scroll=0):
    """a context with a config and no mesh: what a caller converting real images has"""
    c = native.Context(0)
    c.set_config(config(n_cells, scroll), n_angles)
    return c


def geometry(ctx):
    g = ctx._rrcfg
    return dict(scroll=g.scroll_image, theta_min=g.theta_min, theta_inc=g.theta_inc, resolution=g.resolution)


def synthetic(n_frames, n_cells, n_angles, seed):
    """frames cycle through all-zero, all-255 and low noise with sparse strong peaks (peaks at bin 0 and n_cells - 1 too)"""
    rs = np.random.RandomState(seed)
    imgs = rs.randint(0, 30, (n_frames, n_cells, n_angles)).astype(np.uint8)
    peaks = rs.rand(n_frames, n_cells, n_angles) < 0.02
    imgs[peaks] = rs.randint(80, 256, int(peaks.sum()))
    imgs[:, 0, ::3] = 240
    imgs[:, n_cells - 1, 1::3] = 250
    for f in range(n_frames):
        if f % 5 == 3:
            imgs[f] = 0
        elif f % 5 == 4:
            imgs[f] = 255
    return imgs


def assert_frame(got_pts, got_offs, want_pts, want_offs):
    assert np.array_equal(got_offs, want_offs)
    assert len(got_pts) == len(want_pts)
    for k in ("column", "bin", "intensity", "z"):
        assert np.array_equal(got_pts[k], want_pts[k]), k
    r = np.hypot(want_pts["x"].astype(np.float64), want_pts["y"].astype(np.float64))
    for k in ("x", "y"):
        assert np.all(np.abs(got_pts[k].astype(np.float64) - want_pts[k]) <= 1e-6 * r + 1e-6), k


def check_against_ref(ctx, imgs, det, pts, offs):
    g = geometry(ctx)
    for f in range(len(imgs)):
        want_pts, want_offs = R.detect_frame(imgs[f], **det, **g)
        assert_frame(pts[f], offs[f], want_pts, want_offs)


DETECTORS = [dict(method=0, guard_cells=2, train_cells=16, k=12, min_intensity=1, min_bin=0, cfar_scale=3.0),
             dict(method=0, guard_cells=0, train_cells=1, k=1, min_intensity=0, min_bin=5, cfar_scale=1.5),
             dict(method=1, guard_cells=2, train_cells=16, k=12, min_intensity=1, min_bin=0, cfar_scale=3.0),
             dict(method=1, guard_cells=0, train_cells=1, k=40, min_intensity=50, min_bin=3, cfar_scale=0.0)]


@pytest.mark.parametrize("det", DETECTORS, ids=["cfar", "cfar_g0t1_minbin", "k12", "k40_minint"])
@pytest.mark.parametrize("shape", [(16, 200, 400, 0), (1, 100, 37, 5), (64, 300, 400, 123), (2, 3424, 400, 7), (2, 4000, 64, 0)],
                         ids=["16x200x400", "1x100x37_scroll", "64x300x400_scroll", "2x3424x400", "2x4000x64_narrow"])
def test_detectors_match_the_restatement(det, shape):
    n, n_cells, n_angles, scroll = shape
    ctx = conv_ctx(n_cells, n_angles, scroll)
    imgs = synthetic(n, n_cells, n_angles, seed=n_cells + n_angles)
    pts, offs = ctx.detect(imgs, det)
    check_against_ref(ctx, imgs, det, pts, offs)
    assert any(len(p) for p in pts)


def test_simulated_images_device_chain_on_one_stream(native_lib):
    """config-2-sized scene: rr_simulate_batch_device then rr_detect_device / rr_polar_to_cartesian_device on one stream"""
    scene = scenes.config_scene(2)
    cfg = params.kaist_preset(n_reflections=2, n_samples=200, ambient_noise=0)
    ctx = native.Context(0)
    ctx.set_mesh(scene["verts"], scene["faces"], scene["face_object_id"])
    ctx.set_materials(materials_for(scene), scene["object_materials"], 0)
    ctx.set_config(cfg, 400)
    ctx.set_beam_samples(golden_beams(200))
    poses = scenes.trajectory(16, scene["name"])
    n = len(poses)
    s = torch.cuda.Stream(device=DEV)
    imgs = torch.empty((n, cfg.n_cells, 400), dtype=torch.uint8, device=DEV)
    det = dict(DETECTORS[0], cfar_scale=2.0)
    mp = 400 * 200
    pts = torch.empty((n, mp * 24), dtype=torch.uint8, device=DEV)
    offs = torch.empty((n, 401), dtype=torch.int32, device=DEV)
    cart = torch.empty((n, 257, 257), dtype=torch.uint8, device=DEV)
    ctx.simulate_batch_device(poses, imgs.data_ptr(), s.cuda_stream)
    ctx.detect_device(imgs.data_ptr(), n, det, pts.data_ptr(), mp, offs.data_ptr(), s.cuda_stream)
    ctx.polar_to_cartesian_device(imgs.data_ptr(), n, 257, 0.5, cart.data_ptr(), True, s.cuda_stream)
    ctx.synchronize(s.cuda_stream)
    h_imgs = imgs.cpu().numpy()
    h_offs = offs.cpu().numpy().view(np.uint32)
    h_pts = pts.cpu().numpy().view(native.POINT_DTYPE)
    assert h_offs[:, -1].max() <= mp and h_offs[:, -1].min() > 0
    check_against_ref(ctx, h_imgs, det, [h_pts[f, :h_offs[f, -1]] for f in range(n)], h_offs)
    g = geometry(ctx)
    want = np.stack([R.cartesian(h_imgs[f], 257, 0.5, True, **g) for f in range(n)])
    d = np.abs(cart.cpu().numpy().astype(int) - want)
    assert d.max() <= 1 and np.mean(d > 0) <= 1e-3


def test_a_wall_lands_at_its_range_bearing_and_pixel():
    """one wall, 20 m away at bearing +30 deg (to the left), nothing else: the detections sit within one bin of 20 m at that
    bearing and the Cartesian image lights the pixel there, not its mirror image (the sign of theta_inc)"""
    bearing, dist = np.deg2rad(30.0), 20.0
    c, s = np.cos(bearing), np.sin(bearing)
    centre = np.array([dist * c, dist * s, 0.0])
    side = np.array([-s, c, 0.0]) * 3.0                  # the wall is perpendicular to the bearing, 6 m wide, 10 m tall
    up = np.array([0.0, 0.0, 5.0])
    verts = np.array([centre - side - up, centre + side - up, centre + side + up, centre - side + up], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    cfg = params.kaist_preset(n_reflections=1, n_samples=50, ambient_noise=0, signal_denoising=0, n_cells=512)
    ctx = native.Context(0)
    ctx.set_mesh(verts, faces, np.zeros(2, np.uint32))
    ctx.set_materials(params.kaist_materials(), [1], 0)
    ctx.set_config(cfg, 400)
    ctx.set_beam_samples(golden_beams(50))
    img, _, _ = ctx.simulate(np.array([0, 0, 0, 1, 0, 0, 0], np.float32))
    pts, offs = ctx.detect(img, method=1, k=1, min_intensity=1)
    p = pts[0]
    assert len(p) > 0
    # the column whose azimuth points at the wall's centre: yaw -a * 2 pi / 400 = 30 deg (mod 360) -> a = 367
    a = int(round(-bearing / (2 * np.pi / 400))) % 400
    hit = p[p["column"] == (a + cfg.scroll_image) % 400]
    assert len(hit) == 1
    az = np.arctan2(hit["y"][0], hit["x"][0])
    assert abs(az - bearing) <= 2 * np.pi / 400, np.rad2deg(az)
    assert abs(int(hit["bin"][0]) - (dist / cfg.resolution - 0.5)) <= 1.0, hit["bin"]
    assert abs(float(np.hypot(hit["x"][0], hit["y"][0])) - dist) <= 1.5 * cfg.resolution
    bearings = np.rad2deg(np.arctan2(p["y"], p["x"]))
    assert abs(np.median(bearings) - 30.0) <= 2.0, np.median(bearings)     # the lit columns straddle the wall
    assert np.all(np.arctan2(p["y"], p["x"]) > 0)        # every detection is on the left
    cart = ctx.polar_to_cartesian(img, 101, 0.5, bilinear=False)[0]
    cc = 50.0
    i, j = int(round(cc - centre[0] / 0.5)), int(round(cc - centre[1] / 0.5))
    assert cart[i - 1:i + 2, j - 1:j + 2].max() > 0
    jm = int(round(cc + centre[1] / 0.5))                # the mirror image (y -> -y)
    assert cart[i - 2:i + 3, jm - 2:jm + 3].max() == 0
    assert cart.sum() == cart[:, :51].sum()              # nothing on the right half


def test_truncation_keeps_true_totals_and_the_canary():
    n_cells, n_angles = 300, 400
    ctx = conv_ctx(n_cells, n_angles)
    imgs = synthetic(1, n_cells, n_angles, seed=9)
    imgs = np.concatenate([imgs, imgs[::-1]]).copy()
    det = DETECTORS[0]
    want = [R.detect_frame(imgs[f], **det, **geometry(ctx)) for f in range(len(imgs))]
    totals = [int(w[1][-1]) for w in want]
    mp = min(totals) // 2
    assert mp > 10
    n = len(imgs)
    d_imgs = torch.from_numpy(imgs).to(DEV)
    canary = 0xA5
    pts = torch.full((n * mp * 24 + 4096,), canary, dtype=torch.uint8, device=DEV)
    offs = torch.zeros((n, n_angles + 1), dtype=torch.int32, device=DEV)
    ctx.detect_device(d_imgs.data_ptr(), n, det, pts.data_ptr(), mp, offs.data_ptr())
    ctx.synchronize()
    h = pts.cpu().numpy()
    assert np.all(h[n * mp * 24:] == canary)
    got = h[:n * mp * 24].view(native.POINT_DTYPE).reshape(n, mp)
    h_offs = offs.cpu().numpy().view(np.uint32)
    for f in range(n):
        assert_frame(got[f], h_offs[f], want[f][0][:mp], want[f][1])
        assert h_offs[f, -1] == totals[f] > mp
    # the host form reports a truncated frame by name, or keeps its first points when asked to
    with pytest.raises(native.RRError, match="frame 0 has %d detections" % totals[0]):
        ctx.detect(imgs, det, max_points=mp)
    p, o = ctx.detect(imgs, det, max_points=mp, allow_truncation=True)
    assert all(len(x) == mp for x in p) and list(o[:, -1]) == totals
    # count only
    offs.zero_()
    ctx.detect_device(d_imgs.data_ptr(), n, det, None, 0, offs.data_ptr())
    ctx.synchronize()
    assert np.array_equal(offs.cpu().numpy().view(np.uint32), np.stack([w[1] for w in want]))


def test_refusals_return_minus_3_and_write_nothing():
    n_cells, n_angles = 64, 16
    ctx = conv_ctx(n_cells, n_angles)
    L, h = ctx._L, ctx._h
    imgs = synthetic(2, n_cells, n_angles, seed=3)
    d_imgs = torch.from_numpy(imgs).to(DEV)
    pts = torch.full((2 * 32 * 24,), 0x5A, dtype=torch.uint8, device=DEV)
    offs = torch.full((2 * (n_angles + 1) * 4,), 0x5A, dtype=torch.uint8, device=DEV)
    cart = torch.full((2 * 16 * 16,), 0x5A, dtype=torch.uint8, device=DEV)

    def dcfg(**kw):
        c = native.RRDetectConfig()
        L.rr_default_detect_config(C.byref(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def ccfg(width=16, interpolation=1, pixel_size=0.5):
        c = native.RRCartesianConfig()
        c.width, c.interpolation, c.pixel_size = width, interpolation, pixel_size
        return c

    bad_det = [dcfg(method=2), dcfg(method=-1), dcfg(guard_cells=-1), dcfg(guard_cells=1025), dcfg(train_cells=0),
               dcfg(train_cells=1025), dcfg(k=0), dcfg(k=65), dcfg(min_intensity=-1), dcfg(min_intensity=256),
               dcfg(min_bin=-1), dcfg(min_bin=64), dcfg(cfar_scale=-1.0), dcfg(cfar_scale=float("nan")),
               dcfg(cfar_scale=float("inf"))]
    for c in bad_det:
        assert L.rr_detect_device(h, d_imgs.data_ptr(), 2, C.byref(c), pts.data_ptr(), 32, offs.data_ptr(), None) == -3
    good = dcfg()
    for n in (0, 65536, -1):
        assert L.rr_detect_device(h, d_imgs.data_ptr(), n, C.byref(good), pts.data_ptr(), 32, offs.data_ptr(), None) == -3
    assert L.rr_detect_device(h, d_imgs.data_ptr(), 2, C.byref(good), pts.data_ptr(), -1, offs.data_ptr(), None) == -3
    assert L.rr_detect_device(h, None, 2, C.byref(good), pts.data_ptr(), 32, offs.data_ptr(), None) == -3
    assert L.rr_detect_device(h, d_imgs.data_ptr(), 2, None, pts.data_ptr(), 32, offs.data_ptr(), None) == -3
    assert L.rr_detect_device(h, d_imgs.data_ptr(), 2, C.byref(good), None, 32, offs.data_ptr(), None) == -3
    assert L.rr_detect_device(h, d_imgs.data_ptr(), 2, C.byref(good), pts.data_ptr(), 32, None, None) == -3
    assert b"rr_detect_device" in L.rr_last_error(h)
    for c in (ccfg(width=0), ccfg(width=8193), ccfg(interpolation=2), ccfg(pixel_size=0.0), ccfg(pixel_size=-1.0),
              ccfg(pixel_size=float("nan")), ccfg(pixel_size=float("inf"))):
        assert L.rr_polar_to_cartesian_device(h, d_imgs.data_ptr(), 2, C.byref(c), cart.data_ptr(), None) == -3
    assert L.rr_polar_to_cartesian_device(h, d_imgs.data_ptr(), 0, C.byref(ccfg()), cart.data_ptr(), None) == -3
    assert L.rr_polar_to_cartesian_device(h, d_imgs.data_ptr(), 2, C.byref(ccfg()), None, None) == -3
    assert L.rr_polar_to_cartesian_device(h, None, 2, C.byref(ccfg()), cart.data_ptr(), None) == -3
    # host forms: the canaries are host arrays
    h_pts = np.full(2 * 32, 0x5A, np.uint8).repeat(24)
    h_offs = np.full(2 * (n_angles + 1), 0x5A5A5A5A, np.uint32)
    h_cart = np.full(2 * 16 * 16, 0x5A, np.uint8)
    for c in bad_det:
        assert L.rr_detect(h, imgs.ctypes.data, 2, C.byref(c), h_pts.ctypes.data, 32, h_offs.ctypes.data) == -3
    assert L.rr_detect(h, imgs.ctypes.data, 2, C.byref(good), h_pts.ctypes.data, -1, h_offs.ctypes.data) == -3
    assert L.rr_polar_to_cartesian(h, imgs.ctypes.data, 2, C.byref(ccfg(width=0)), h_cart.ctypes.data) == -3
    torch.cuda.synchronize()
    assert np.all(h_pts == 0x5A) and np.all(h_offs == 0x5A5A5A5A) and np.all(h_cart == 0x5A)
    for t in (pts, offs, cart):
        assert bool((t == 0x5A).all())
    # without a config: -2
    bare = native.Context(0)
    assert bare._L.rr_detect_device(bare._h, d_imgs.data_ptr(), 2, C.byref(good), pts.data_ptr(), 32, offs.data_ptr(), None) == -2
    assert bare._L.rr_polar_to_cartesian_device(bare._h, d_imgs.data_ptr(), 2, C.byref(ccfg()), cart.data_ptr(), None) == -2


def test_a_context_without_a_mesh_converts_images():
    ctx = conv_ctx(3424, 400)
    imgs = synthetic(1, 3424, 400, seed=5)               # a noisy "real" image
    pts, offs = ctx.detect(imgs, DETECTORS[2])
    assert len(pts[0]) == int(offs[0, -1]) > 0
    cart = ctx.polar_to_cartesian(imgs, 128, 1.0)
    assert cart.shape == (1, 128, 128) and cart.any()


@pytest.mark.parametrize("width,bilinear,scroll", [(257, False, 0), (256, False, 17), (255, True, 0), (300, True, 399), (1, True, 0), (2, False, 3)])
def test_cartesian_matches_the_restatement(width, bilinear, scroll):
    n_cells = 700
    ctx = conv_ctx(n_cells, 400, scroll)
    imgs = synthetic(3, n_cells, 400, seed=width)
    imgs[0] = np.random.RandomState(1).randint(0, 256, imgs[0].shape)     # noise: every rounding shows
    ps = 2 * n_cells * ctx._rrcfg.resolution / width                         # the image reaches a little past the last bin
    got = ctx.polar_to_cartesian(imgs, width, ps, bilinear)
    g = geometry(ctx)
    for f in range(len(imgs)):
        if bilinear:
            want = R.cartesian(imgs[f], width, ps, True, **g)
            d = np.abs(got[f].astype(int) - want)
            assert d.max() <= 1 and np.mean(d > 0) <= 1e-3, (d.max(), np.mean(d > 0))
        else:
            want, b, a, outside = R.cartesian(imgs[f], width, ps, False, with_cells=True, **g)
            bad = np.nonzero(got[f] != want)
            assert len(bad[0]) <= max(1, 1e-3 * want.size), len(bad[0])
            sc = g["scroll"] % 400
            for i, j in zip(*bad):                       # a flipped rounding reads a neighbouring cell
                if outside[i, j]:
                    ok = {0} | {int(imgs[f][n_cells - 1, (a[i, j] + da + sc) % 400]) for da in (-1, 0, 1)}
                else:
                    ok = {int(imgs[f][min(max(b[i, j] + db, 0), n_cells - 1), (a[i, j] + da + sc) % 400])
                          for db in (-1, 0, 1) for da in (-1, 0, 1)}
                assert int(got[f][i, j]) in ok, (i, j)


def test_two_streams_convert_different_batches_at_once():
    n_cells = 500
    ctx = conv_ctx(n_cells, 400, 11)
    a = synthetic(16, n_cells, 400, seed=21)
    b = synthetic(16, n_cells, 400, seed=22)[::-1].copy()
    det = DETECTORS[2]
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    out = []
    for imgs, s in ((a, s1), (b, s2)):
        d = torch.from_numpy(imgs).to(DEV)
        torch.cuda.synchronize()
        pts = torch.empty((16, 400 * 12 * 24), dtype=torch.uint8, device=DEV)
        offs = torch.empty((16, 401), dtype=torch.int32, device=DEV)
        cart = torch.empty((16, 200, 200), dtype=torch.uint8, device=DEV)
        out.append((imgs, d, pts, offs, cart, s))
    for imgs, d, pts, offs, cart, s in out:
        ctx.detect_device(d.data_ptr(), 16, det, pts.data_ptr(), 400 * 12, offs.data_ptr(), s.cuda_stream)
        ctx.polar_to_cartesian_device(d.data_ptr(), 16, 200, 0.3, cart.data_ptr(), True, s.cuda_stream)
    torch.cuda.synchronize()
    g = geometry(ctx)
    for imgs, d, pts, offs, cart, s in out:
        h_offs = offs.cpu().numpy().view(np.uint32)
        h_pts = pts.cpu().numpy().view(native.POINT_DTYPE)
        check_against_ref(ctx, imgs, det, [h_pts[f, :h_offs[f, -1]] for f in range(16)], h_offs)
        want = np.stack([R.cartesian(imgs[f], 200, 0.3, True, **g) for f in range(16)])
        dd = np.abs(cart.cpu().numpy().astype(int) - want)
        assert dd.max() <= 1 and np.mean(dd > 0) <= 1e-3


def test_conversions_leave_the_frame_path_alone():
    s = scenes.box12()
    cfg = params.kaist_preset(n_reflections=2, ambient_noise=0)
    ctx = native.Context(0)
    ctx.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    ctx.set_materials(params.kaist_materials(), s["object_materials"], 0)
    ctx.set_config(cfg)
    ctx.set_beam_samples(golden_beams(100))
    pose = scenes.default_pose("box12")
    before, f_before, _ = ctx.simulate(pose, want_f32=True)
    imgs = np.stack([before, synthetic(1, cfg.n_cells, 400, seed=2)[0]])
    for det in DETECTORS:
        ctx.detect(imgs, det)
    ctx.polar_to_cartesian(imgs, 512, 0.2, True)
    ctx.polar_to_cartesian(imgs, 99, 0.7, False)
    after, f_after, _ = ctx.simulate(pose, want_f32=True)
    assert np.array_equal(before, after) and np.array_equal(f_before, f_after)
    assert before.any()


def test_radar_facade_point_clouds_and_cartesian():
    """RadarHIP: simulatePointClouds (simulate + detect on one stream, no image to the host) equals toPointCloud of the
    images simulateBatch delivers, and both equal the restatement; toCartesian equals the context's conversion"""
    from radarays_ros_amd import radar
    s = scenes.box12()
    r = radar.RadarHIP(s["verts"], s["faces"], s["face_object_id"])
    r.loadParams(params.kaist_materials(), s["object_materials"], 0)
    r.updateDynCfg(params.kaist_preset(n_reflections=2, ambient_noise=0))
    r.setBeamSamples(golden_beams(100))
    poses = np.stack([scenes.default_pose("box12"), scenes.yaw_pose(1.0, 1.5, 0.2, 1.0), scenes.yaw_pose(0.5, 1.0, 0.2, -2.0)])
    clouds = r.simulatePointClouds(poses, method="kstrongest", k=4)
    imgs = r.simulateBatch(poses)
    g = geometry(r.context)
    assert len(clouds) == len(imgs) == 3
    for cl, im in zip(clouds, imgs):
        want, offs = R.detect_frame(im.data, method=1, k=4, **g)
        assert_frame(cl, offs, want, offs)
        assert_frame(r.toPointCloud(im, method=1, k=4), offs, want, offs)
        assert len(cl) > 0
    cart = r.toCartesian(imgs[0], 64, 0.2)
    assert (cart.height, cart.width, cart.encoding) == (64, 64, "mono8")
    assert np.array_equal(cart.data, r.context.polar_to_cartesian(imgs[0].data, 64, 0.2, True)[0])
