"""Windowed CFAR on the GPU (rr_window.hip) against the numpy restatement of its definition (tests/window_ref.py): points, order,
offsets and mask bit for bit, x and y to the tolerance of test_gpu_detect.assert_frame.  The shapes are the smallest that reach every
edge: the byte-load path with the seam wrapped, a window taller than the image, a window that is the whole circle, several strips and
frames, and bin counts on both sides of the kernel's range step."""
import ctypes as C

import numpy as np
import pytest

import window_ref as W
from common import golden_beams
from radarays_ros_amd import native, params, scenes
from test_gpu_detect import assert_frame, conv_ctx, geometry
from test_window_host import BAD, raw_cfg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"

WINDOWS = {"default": dict(),
           "g0t1": dict(guard_range=0, train_range=1, guard_azimuth=0, train_azimuth=1, rank_permille=500, scale=1.5, min_intensity=0, min_bin=5)}
METHODS = {"ca": W.CA, "go": W.GO, "so": W.SO, "os": W.OS}


def frames(n_frames, n_cells, n_angles, seed):
    """frame 0: low noise, sparse strong peaks (bin 0 and the last bin too) and a wall across every column; then all-zero and all-255
    frames in turn, as test_gpu_detect.synthetic has them"""
    rs = np.random.RandomState(seed)
    imgs = rs.randint(0, 30, (n_frames, n_cells, n_angles)).astype(np.uint8)
    peaks = rs.rand(n_frames, n_cells, n_angles) < 0.02
    imgs[peaks] = rs.randint(80, 256, int(peaks.sum()))
    imgs[:, 0, ::3] = 240
    imgs[:, n_cells - 1, 1::3] = 250
    imgs[:, n_cells // 2:n_cells // 2 + 6, :] = 200
    for f in range(n_frames):
        if f % 3 == 1:
            imgs[f] = 0
        elif f % 3 == 2:
            imgs[f] = 255
    return imgs


SHAPES = {"2x64x37_scroll": (2, 64, 37, 5), "1x20x16_short": (1, 20, 16, 0), "1x40x7_circle": (1, 40, 7, 0), "3x300x400_scroll": (3, 300, 400, 123)}
# bin counts on the seams of the range step (256 bins for both windows: test_the_seam_shapes_sit_on_the_step), one strip and a column
SEAMS = {"%dx17" % n: (3 if n == 257 else 1, n, 17, 3) for n in (255, 256, 257, 511, 512, 513)}
# the narrower strips of taller images: 8 columns past 1024 bins (step 512: one step and 7 bins), 4 past 2048 (step 1024: two and one bin), with
# 16-byte row loads (strips that do not start on a multiple of 16) and with byte loads (a last strip of one column)
SEAMS.update({"1031x32": (1, 1031, 32, 3), "2049x48": (1, 2049, 48, 40), "2049x9": (2, 2049, 9, 2)})
_REF = {}


def reference(shape_id, window_id):
    """the frames of a shape and, per frame, the four masks of the restatement under a window: computed once, shared, never written to"""
    key = (shape_id, window_id)
    if key not in _REF:
        n, n_cells, n_angles, scroll = {**SHAPES, **SEAMS}[shape_id]
        imgs = frames(n, n_cells, n_angles, seed=n_cells + n_angles)
        imgs.setflags(write=False)
        _REF[key] = (imgs, [W.masks(img, WINDOWS[window_id]) for img in imgs])
    return _REF[key]


def check(ctx, imgs, masks, method, pts, offs, got_mask=None):
    g = geometry(ctx)
    for f in range(len(imgs)):
        want_pts, want_offs = W.points_of(imgs[f], masks[f][method], **g)
        assert_frame(pts[f], offs[f], want_pts, want_offs)
        if got_mask is not None:
            assert np.array_equal(got_mask[f], np.where(masks[f][method], 255, 0).astype(np.uint8))


def test_the_seam_shapes_sit_on_the_step():
    for w in WINDOWS.values():
        for m in METHODS.values():
            tile = lambda n, a: native.detect_window_tile_sizes(dict(w, method=m), n, a)[:2]      # noqa: E731
            assert tile(513, 17) == (256, 16) and tile(1031, 32) == (512, 8) and tile(2049, 48) == tile(2049, 9) == (1024, 4)


# windows whose step does not fit 64 KB of LDS: strips below 16 columns at any height, the large-LDS launch.  (Gr + Tr, Ga + Ta) ->
# 2049 x 3 and 401 x 41 cells
BIG = {"tall": dict(guard_range=24, train_range=1000, guard_azimuth=0, train_azimuth=1, scale=1.2, rank_permille=900),
       "wide_tall": dict(guard_range=3, train_range=197, guard_azimuth=4, train_azimuth=16, scale=1.2, rank_permille=900)}


@pytest.mark.parametrize("window", list(BIG))
def test_large_windows_take_narrow_strips_and_more_than_64_kb(window):
    n_cells, n_angles = (300, 16) if window == "tall" else (50, 48)
    w = BIG[window]
    imgs = frames(1, n_cells, n_angles, seed=31)
    masks = [W.masks(imgs[0], w)]
    ctx = conv_ctx(n_cells, n_angles, 3)
    narrow = big = found = 0
    for m in METHODS.values():
        rows, cols, hr, hc = native.detect_window_tile_sizes(dict(w, method=m), n_cells, n_angles)
        wq = 16 + 2 * (-(-hc // 16) * 16) if cols == 16 else -(-(15 + 2 * hc + cols) // 16) * 16
        lds = (rows + 2 * hr) * (wq + (0 if m == W.OS else 4 * cols))
        narrow += cols < 16
        big += lds > 64 * 1024
        pts, offs, mask = ctx.detect_window(imgs, dict(w, method=m), mask=True)
        check(ctx, imgs, masks, m, pts, offs, mask)
        found += len(pts[0])
    assert found > 0
    if window == "tall":                                 # every method: a strip below 16 columns and a step above 64 KB
        assert narrow == 4 and big == 4


def test_an_unaligned_base_takes_byte_loads_and_the_same_tile():
    """n_angles % 16 == 0 and a device base that is not 16-byte aligned: the byte-load path, the reported tile and the same result"""
    shape, window = "3x300x400_scroll", "default"
    n, n_cells, n_angles, scroll = SHAPES[shape]
    imgs, masks = reference(shape, window)
    ctx = conv_ctx(n_cells, n_angles, scroll)
    buf = torch.zeros(imgs.size + 16, dtype=torch.uint8, device=DEV)
    off = 5 if buf.data_ptr() % 16 == 0 else 0
    buf[off:off + imgs.size] = torch.from_numpy(imgs.copy()).reshape(-1).to(DEV)
    assert (buf.data_ptr() + off) % 16 != 0
    mp = n_cells * n_angles
    for m in (W.CA, W.OS):
        pts = torch.zeros((n, mp * 24), dtype=torch.uint8, device=DEV)
        offs = torch.zeros((n, n_angles + 1), dtype=torch.int32, device=DEV)
        mask = torch.zeros((n, n_cells, n_angles), dtype=torch.uint8, device=DEV)
        ctx.detect_window_device(buf.data_ptr() + off, n, dict(method=m), pts.data_ptr(), mp, offs.data_ptr(), mask.data_ptr())
        ctx.synchronize()
        h_offs = offs.cpu().numpy().view(np.uint32)
        h_pts = pts.cpu().numpy().view(native.POINT_DTYPE)
        check(ctx, imgs, masks, m, [h_pts[f, :h_offs[f, -1]] for f in range(n)], h_offs, mask.cpu().numpy())


@pytest.mark.parametrize("method", list(METHODS))
@pytest.mark.parametrize("window", list(WINDOWS))
@pytest.mark.parametrize("shape", list(SHAPES) + list(SEAMS))
def test_window_detectors_match_the_restatement(shape, window, method):
    n, n_cells, n_angles, scroll = {**SHAPES, **SEAMS}[shape]
    imgs, masks = reference(shape, window)
    ctx = conv_ctx(n_cells, n_angles, scroll)
    cfg = dict(WINDOWS[window], method=METHODS[method])
    pts, offs, mask = ctx.detect_window(imgs, cfg, mask=True)
    check(ctx, imgs, masks, METHODS[method], pts, offs, mask)
    if window == "default" and n_cells >= 64:
        assert any(len(p) for p in pts)


def test_ca_without_an_azimuth_window_is_rr_detect_on_the_same_buffer():
    n_cells, n_angles = 300, 400
    ctx = conv_ctx(n_cells, n_angles, 7)
    imgs = frames(3, n_cells, n_angles, seed=4)
    d = torch.from_numpy(imgs).to(DEV)
    mp = n_cells * n_angles
    out = []
    for win in (False, True):
        pts = torch.zeros((3, mp * 24), dtype=torch.uint8, device=DEV)
        offs = torch.zeros((3, n_angles + 1), dtype=torch.int32, device=DEV)
        if win:
            ctx.detect_window_device(d.data_ptr(), 3, dict(method=0, guard_range=2, train_range=16, guard_azimuth=0, train_azimuth=0, scale=2.0),
                                     pts.data_ptr(), mp, offs.data_ptr())
        else:
            ctx.detect_device(d.data_ptr(), 3, dict(method=0, guard_cells=2, train_cells=16, cfar_scale=2.0), pts.data_ptr(), mp, offs.data_ptr())
        ctx.synchronize()
        out.append((pts.cpu().numpy(), offs.cpu().numpy()))
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][0], out[1][0])
    assert out[0][1][0, -1] > 0


def test_truncation_count_only_and_the_mask_is_the_scatter_of_the_points():
    shape, window = "3x300x400_scroll", "default"
    n, n_cells, n_angles, scroll = SHAPES[shape]
    imgs, masks = reference(shape, window)
    ctx = conv_ctx(n_cells, n_angles, scroll)
    g = geometry(ctx)
    want = [W.points_of(imgs[f], masks[f][W.OS], **g) for f in range(n)]
    totals = [int(w[1][-1]) for w in want]
    mp = totals[0] // 2
    assert mp > 10
    d_imgs = torch.from_numpy(imgs.copy()).to(DEV)
    canary = 0xA5
    pts = torch.full((n * mp * 24 + 4096,), canary, dtype=torch.uint8, device=DEV)
    offs = torch.zeros((n, n_angles + 1), dtype=torch.int32, device=DEV)
    mask = torch.full((n, n_cells, n_angles), canary, dtype=torch.uint8, device=DEV)
    ctx.detect_window_device(d_imgs.data_ptr(), n, None, pts.data_ptr(), mp, offs.data_ptr(), mask.data_ptr())
    ctx.synchronize()
    h = pts.cpu().numpy()
    assert np.all(h[n * mp * 24:] == canary)
    got = h[:n * mp * 24].view(native.POINT_DTYPE).reshape(n, mp)
    h_offs = offs.cpu().numpy().view(np.uint32)
    for f in range(n):
        k = min(mp, totals[f])
        assert_frame(got[f][:k], h_offs[f], want[f][0][:k], want[f][1])
    assert h_offs[0, -1] == totals[0] > mp
    h_mask = mask.cpu().numpy()
    for f in range(n):                                   # the mask is whole also where the points were cut
        scatter = np.zeros((n_cells, n_angles), np.uint8)
        scatter[want[f][0]["bin"], want[f][0]["column"]] = 255
        assert np.array_equal(h_mask[f], scatter)
    with pytest.raises(native.RRError, match="frame 0 has %d detections" % totals[0]):
        ctx.detect_window(imgs, None, max_points=mp)
    p, o = ctx.detect_window(imgs, None, max_points=mp, allow_truncation=True)
    assert len(p[0]) == mp and list(o[:, -1]) == totals
    # count only: no point buffer, the same offsets
    offs.zero_()
    ctx.detect_window_device(d_imgs.data_ptr(), n, None, None, 0, offs.data_ptr())
    ctx.synchronize()
    assert np.array_equal(offs.cpu().numpy().view(np.uint32), np.stack([w[1] for w in want]))


def test_the_wall_scene_is_one_component():
    img, wall = W.wall_scene()
    ctx = conv_ctx(200, 37)
    cfg = dict(guard_range=2, train_range=16, guard_azimuth=1, train_azimuth=2, rank_permille=500, scale=4.0)
    pts, offs, mask = ctx.detect_window(img, cfg, mask=True)
    assert np.array_equal(mask[0] == 255, wall) and len(pts[0]) == 444
    assert len(ctx.detect(img, method=0, guard_cells=2, train_cells=16, cfar_scale=4.0)[0][0]) < 444
    out = ctx.label_components(mask, native.components_config(200, 37, threshold=255, connectivity=4, wrap_x=True, max_components=4))
    assert list(out["counts"][0]) == [1, 0]
    assert int(out["comps"][0]["n_pixels"][0]) == 444


def test_refusals_return_minus_3_and_write_nothing():
    n_cells, n_angles = 64, 64
    ctx = conv_ctx(n_cells, n_angles)
    L, h = ctx._L, ctx._h
    imgs = frames(2, n_cells, n_angles, seed=3)
    d_imgs = torch.from_numpy(imgs).to(DEV)
    pts = torch.full((2 * 32 * 24,), 0x5A, dtype=torch.uint8, device=DEV)
    offs = torch.full((2 * (n_angles + 1) * 4,), 0x5A, dtype=torch.uint8, device=DEV)
    mask = torch.full((2 * n_cells * n_angles,), 0x5A, dtype=torch.uint8, device=DEV)
    h_pts = np.full(2 * 32 * 24, 0x5A, np.uint8)
    h_offs = np.full(2 * (n_angles + 1), 0x5A5A5A5A, np.uint32)
    h_mask = np.full(2 * n_cells * n_angles, 0x5A, np.uint8)

    def dev(c, n=2, imgs_p=d_imgs.data_ptr(), pts_p=pts.data_ptr(), mp=32, offs_p=offs.data_ptr()):
        return L.rr_detect_window_device(h, imgs_p, n, c, pts_p, mp, offs_p, mask.data_ptr(), None)

    def host(c, n=2, mp=32):
        return L.rr_detect_window(h, imgs.ctypes.data, n, c, h_pts.ctypes.data, mp, h_offs.ctypes.data, h_mask.ctypes.data)

    for kw in BAD:
        c = C.byref(raw_cfg(L, **kw))
        assert dev(c) == -3 and host(c) == -3, kw
    good = C.byref(raw_cfg(L))
    for n in (0, 65536, -1):
        assert dev(good, n=n) == -3 and host(good, n=n) == -3
    assert dev(good, mp=-1) == -3 and host(good, mp=-1) == -3
    assert dev(good, imgs_p=None) == -3 and dev(None) == -3 and dev(good, pts_p=None) == -3 and dev(good, offs_p=None) == -3
    assert b"rr_detect_window_device" in L.rr_last_error(h)
    torch.cuda.synchronize()
    assert np.all(h_pts == 0x5A) and np.all(h_offs == 0x5A5A5A5A) and np.all(h_mask == 0x5A)
    for t in (pts, offs, mask):
        assert bool((t == 0x5A).all())
    bare = native.Context(0)
    assert bare._L.rr_detect_window_device(bare._h, d_imgs.data_ptr(), 2, good, pts.data_ptr(), 32, offs.data_ptr(), None, None) == -2


def test_two_streams_convert_different_batches_at_once():
    n_cells, n_angles = 130, 400
    ctx = conv_ctx(n_cells, n_angles, 11)
    batches = [frames(4, n_cells, n_angles, seed=21), frames(4, n_cells, n_angles, seed=22)[::-1].copy()]
    cfgs = [dict(method=W.OS), dict(method=W.GO)]
    out = []
    for imgs in batches:
        d = torch.from_numpy(imgs).to(DEV)
        pts = torch.empty((4, n_cells * n_angles * 24), dtype=torch.uint8, device=DEV)
        offs = torch.empty((4, n_angles + 1), dtype=torch.int32, device=DEV)
        mask = torch.empty((4, n_cells, n_angles), dtype=torch.uint8, device=DEV)
        out.append((imgs, d, pts, offs, mask, torch.cuda.Stream(device=DEV)))
    torch.cuda.synchronize()
    for (imgs, d, pts, offs, mask, s), cfg in zip(out, cfgs):
        ctx.detect_window_device(d.data_ptr(), 4, cfg, pts.data_ptr(), n_cells * n_angles, offs.data_ptr(), mask.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()
    for (imgs, d, pts, offs, mask, s), cfg in zip(out, cfgs):
        h_offs = offs.cpu().numpy().view(np.uint32)
        h_pts = pts.cpu().numpy().view(native.POINT_DTYPE)
        masks = [W.masks(img, {}) for img in imgs]
        check(ctx, imgs, masks, cfg["method"], [h_pts[f, :h_offs[f, -1]] for f in range(4)], h_offs, mask.cpu().numpy())


def test_a_simulate_batch_in_flight_is_unchanged_by_a_concurrent_call():
    s = scenes.box12()
    cfg = params.kaist_preset(n_reflections=2, ambient_noise=0)
    ctx = native.Context(0)
    ctx.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    ctx.set_materials(params.kaist_materials(), s["object_materials"], 0)
    ctx.set_config(cfg)
    ctx.set_beam_samples(golden_beams(100))
    poses = np.stack([scenes.default_pose("box12")] * 4)
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    alone = torch.empty((4, cfg.n_cells, 400), dtype=torch.uint8, device=DEV)
    ctx.simulate_batch_device(poses, alone.data_ptr(), s1.cuda_stream)
    ctx.synchronize(s1.cuda_stream)
    other = torch.from_numpy(frames(4, cfg.n_cells, 400, seed=2)).to(DEV)
    offs = torch.empty((4, 401), dtype=torch.int32, device=DEV)
    mask = torch.empty((4, cfg.n_cells, 400), dtype=torch.uint8, device=DEV)
    beside = torch.empty_like(alone)
    torch.cuda.synchronize()
    ctx.simulate_batch_device(poses, beside.data_ptr(), s1.cuda_stream)
    ctx.detect_window_device(other.data_ptr(), 4, dict(WINDOWS["g0t1"], method=W.OS), None, 0, offs.data_ptr(), mask.data_ptr(), s2.cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(alone, beside) and bool(alone.any())
    h_other = other.cpu().numpy()
    want = W.masks(h_other[0], WINDOWS["g0t1"])[W.OS]
    assert np.array_equal(mask[0].cpu().numpy() == 255, want) and int(offs[0, -1]) == int(want.sum())


def test_radar_facade_window_calls():
    from radarays_ros_amd import radar
    s = scenes.box12()
    r = radar.RadarHIP(s["verts"], s["faces"], s["face_object_id"])
    r.loadParams(params.kaist_materials(), s["object_materials"], 0)
    r.updateDynCfg(params.kaist_preset(n_reflections=2, ambient_noise=0))
    r.setBeamSamples(golden_beams(100))
    poses = np.stack([scenes.default_pose("box12"), scenes.yaw_pose(1.0, 1.5, 0.2, 1.0)])
    win = dict(method="ca", scale=2.0)
    clouds = r.simulatePointClouds(poses, window=win)
    imgs = r.simulateBatch(poses)
    g = geometry(r.context)
    for cl, im in zip(clouds, imgs):
        want, offs = W.points_of(im.data, W.masks(im.data, dict(scale=2.0))[W.CA], **g)
        assert_frame(cl, offs, want, offs)
        got, mask = r.detectWindow(im, mask=True, **win)
        assert_frame(got, offs, want, offs)
        assert int((mask == 255).sum()) == len(want) > 0
    assert len(r.simulatePointClouds(poses[:1])[0]) == len(r.toPointCloud(imgs[0]))       # the default path is rr_detect's
