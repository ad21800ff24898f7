"""Azimuth registration on the GPU (rr_align.hip: rr_align_images_device, rr_align_images, rr_simulate_batch_align) against
the numpy restatement of its definition (tests/align_ref.py).

Bounds.  The curve, shift, n_best, xcorr, sse and the four sums are integers and compared bit for bit.  ncc and psnr within
1e-12 absolute: their inputs are exact integers, |ncc| <= 1, and there are at most four f64 roundings (psnr below 100 dB: a
few ulps of log10 are 1e-14)."""
import numpy as np
import pytest

import align_ref as A
from common import golden_beams, materials_for
from radarays_ros_amd import native, params, scenes
from test_gpu_metrics import conv_ctx, dark, image_set

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
TOL = 1e-12
POISON = 0x5A5A5A5A5A5A5A5A
INT_FIELDS = ("shift", "n_best", "xcorr", "sse", "sum_x", "sum_xx", "sum_r", "sum_rr")
REC_BYTES = native.ALIGN_DTYPE.itemsize


def run_device(ctx, imgs, ref, cb=0, ce=None, offset=0, want_curve=True):
    """the images (and the reference) at `offset` bytes past an aligned device allocation, the curve buffer poisoned ->
    (records, curve int64 [n][n_angles])"""
    n, n_angles = len(imgs), imgs.shape[2]
    buf = torch.zeros(imgs.size + offset + 16, dtype=torch.uint8, device=DEV)
    buf[offset:offset + imgs.size] = torch.from_numpy(imgs.ravel()).to(DEV)
    rbuf = torch.zeros(ref.size + offset + 16, dtype=torch.uint8, device=DEV)
    rbuf[offset:offset + ref.size] = torch.from_numpy(ref.ravel()).to(DEV)
    d_curve = torch.full((n, n_angles), POISON, dtype=torch.int64, device=DEV) if want_curve else None
    torch.cuda.synchronize()
    rec = ctx.align_images_device(buf.data_ptr() + offset, n, rbuf.data_ptr() + offset, cb, ce, None if d_curve is None else d_curve.data_ptr())
    return rec, (None if d_curve is None else d_curve.cpu().numpy())


_WANT = {}


def expected(imgs, ref, key, cb=0, ce=None):
    """the restatement's records (with their curves), computed once per image set and window"""
    if key not in _WANT:
        _WANT[key] = [A.align(im, ref, cb, ce) for im in imgs]
    return _WANT[key]


def assert_records(rec, curve, want):
    assert len(rec) == len(want)
    for k, w in enumerate(want):
        r = rec[k]
        print("image %d: shift %d (want %d) n_best %d xcorr %d sse %d psnr %r (want %r) ncc %.15f (diff %.2e)" % (
            k, r["shift"], w["shift"], r["n_best"], r["xcorr"], r["sse"], float(r["psnr"]), w["psnr"], r["ncc"], abs(r["ncc"] - w["ncc"])))
        if curve is not None:
            assert np.array_equal(curve[k], w["curve"]), (k, np.flatnonzero(curve[k] != w["curve"])[:8])
        for f in INT_FIELDS:
            assert int(r[f]) == w[f], (k, f, int(r[f]), w[f])
        assert abs(r["ncc"] - w["ncc"]) <= TOL, (k, r["ncc"], w["ncc"])
        if w["sse"] == 0:
            assert np.isinf(r["psnr"]) and r["psnr"] > 0, (k, r["psnr"])
        else:
            assert abs(r["psnr"] - w["psnr"]) <= TOL, (k, r["psnr"], w["psnr"])


def shape_set(n_cells, n_angles):
    """three images: the reference rolled by 11 columns, a 30 % corrupted copy, other noise"""
    base, ref = image_set(4, n_cells, n_angles, seed=n_cells + n_angles)
    return np.stack([np.roll(ref, 11, axis=1), base[0], base[3]]), ref


# (40, 600): more than 512 azimuths, so a tile row meets two column groups of reference tiles
@pytest.mark.parametrize("shape", [(64, 37), (100, 400), (3424, 400), (40, 600)], ids=["64x37", "100x400", "3424x400", "40x600_two_column_groups"])
def test_curve_and_records_match_the_restatement(shape):
    n_cells, n_angles = shape
    ctx = conv_ctx(n_cells, n_angles)
    imgs, ref = shape_set(n_cells, n_angles)
    want = expected(imgs, ref, ("set", shape))
    rec, curve = run_device(ctx, imgs, ref)
    assert_records(rec, curve, want)
    r0 = rec[0]
    assert r0["shift"] == n_angles - 11 and r0["sse"] == 0 and np.isinf(r0["psnr"]) and r0["psnr"] > 0 and r0["n_best"] == 1
    assert abs(r0["ncc"] - 1.0) <= TOL
    # with the full window, the SSE at shift 0 is rr_score_images_device's
    d_imgs, d_ref = torch.from_numpy(imgs).to(DEV), torch.from_numpy(ref).to(DEV)
    _, sse = ctx.score_images_device(d_imgs.data_ptr(), len(imgs), d_ref.data_ptr(), want_sse=True)
    for k in range(len(imgs)):
        assert int(rec["sum_xx"][k]) + int(rec["sum_rr"][k]) - 2 * int(curve[k][0]) == int(sse[k]), k
    # two identical calls return identical bytes
    again, curve2 = run_device(ctx, imgs, ref)
    assert rec.tobytes() == again.tobytes() and curve.tobytes() == curve2.tobytes()
    # without a curve buffer, and the host form
    no_curve, _ = run_device(ctx, imgs, ref, want_curve=False)
    assert no_curve.tobytes() == rec.tobytes()
    h_rec, h_curve = ctx.align_images(imgs, ref, want_curve=True)
    assert h_rec.tobytes() == rec.tobytes() and np.array_equal(h_curve, curve)
    assert ctx.align_images(imgs, ref).tobytes() == rec.tobytes()
    if shape == (3424, 400):
        # 24 images: the launch gives a workgroup 16 strips (1024 cells), the largest K-chunk
        many = np.stack([imgs[k % 3] for k in range(24)])
        rec24, curve24 = run_device(ctx, many, ref)
        assert_records(rec24, curve24, [want[k % 3] for k in range(24)])
    ctx.close()


@pytest.mark.parametrize("shape", [(64, 37), (100, 400)], ids=["64x37", "100x400"])
@pytest.mark.parametrize("a0,a1", [(5, 30), (30, 5)], ids=["a0<a1", "a1<a0_wraps"])
def test_single_pixels(shape, a0, a1):
    """x has one pixel of value 3 at (c0, a0), r one of value 5 at (c0, a1): 15 at s = (a1 - a0) mod n_angles, 0 elsewhere
    (a swapped row and column only flips the sign of the shift)"""
    n_cells, n_angles = shape
    ctx = conv_ctx(n_cells, n_angles)
    c0 = n_cells - 3
    x, r = np.zeros((1, n_cells, n_angles), np.uint8), np.zeros((n_cells, n_angles), np.uint8)
    x[0, c0, a0], r[c0, a1] = 3, 5
    rec, curve = run_device(ctx, x, r)
    want = np.zeros(n_angles, np.int64)
    want[(a1 - a0) % n_angles] = 15
    assert np.array_equal(curve[0], want), np.flatnonzero(curve[0])
    assert rec["shift"][0] == (a1 - a0) % n_angles and rec["n_best"][0] == 1 and rec["xcorr"][0] == 15 and rec["sse"][0] == 4
    assert (rec["sum_x"][0], rec["sum_xx"][0], rec["sum_r"][0], rec["sum_rr"][0]) == (3, 9, 5, 25)
    assert_records(rec, curve, [A.align(x[0], r)])
    ctx.close()


def test_constant_images():
    """all-0 against all-0 at full size, 24 images (the largest magnitude in the signed domain over the largest K-chunk), and
    all-255 against all-255: every shift ties"""
    n_cells, n_angles = 3424, 400
    n_px = n_cells * n_angles
    ctx = conv_ctx(n_cells, n_angles)
    zero = np.zeros((n_cells, n_angles), np.uint8)
    for n in (1, 24):
        rec, curve = run_device(ctx, np.zeros((n, n_cells, n_angles), np.uint8), zero)
        assert not curve.any()
        for f, v in (("shift", 0), ("n_best", n_angles), ("xcorr", 0), ("sse", 0), ("sum_x", 0), ("sum_xx", 0), ("sum_r", 0), ("sum_rr", 0)):
            assert np.all(rec[f] == v), (n, f, rec[f])
        assert np.all(rec["ncc"] == 0.0) and np.all(np.isinf(rec["psnr"])) and np.all(rec["psnr"] > 0)
    full = np.full((n_cells, n_angles), 255, np.uint8)
    imgs = np.stack([full, zero])
    rec, curve = run_device(ctx, imgs, full)
    assert np.all(curve[0] == 255 * 255 * n_px) and not curve[1].any()
    assert rec["shift"][0] == 0 and rec["n_best"][0] == n_angles and rec["xcorr"][0] == 255 * 255 * n_px and rec["sse"][0] == 0
    assert rec["ncc"][0] == 0.0 and rec["sum_x"][0] == 255 * n_px and rec["sum_rr"][0] == 255 * 255 * n_px
    assert rec["n_best"][1] == n_angles and rec["sse"][1] == 255 * 255 * n_px
    ctx.close()
    ctx = conv_ctx(64, 37)
    full = np.full((64, 37), 255, np.uint8)
    rs = np.random.RandomState(4)
    imgs = np.stack([full, dark(full.shape, rs)])
    rec, curve = run_device(ctx, imgs, full)
    assert_records(rec, curve, [A.align(im, full) for im in imgs])
    assert rec["n_best"][0] == 37 and rec["n_best"][1] == 37             # against a constant reference every shift ties
    ctx.close()


@pytest.mark.parametrize("win", [(5, 64), (0, 1), (63, 64)], ids=["5_64", "0_1", "63_64"])
def test_cell_windows(win):
    n_cells, n_angles = 64, 37
    ctx = conv_ctx(n_cells, n_angles)
    imgs, ref = shape_set(n_cells, n_angles)
    rec, curve = run_device(ctx, imgs, ref, *win)
    assert_records(rec, curve, expected(imgs, ref, ("win", win), *win))
    assert rec["shift"][0] == n_angles - 11 and rec["sse"][0] == 0
    assert int(rec["sum_x"][1]) == int(imgs[1][win[0]:win[1]].sum(dtype=np.int64))
    ctx.close()


@pytest.mark.parametrize("offset", [1, 3])
def test_images_at_odd_byte_offsets(offset):
    n_cells, n_angles = 100, 400
    ctx = conv_ctx(n_cells, n_angles)
    imgs, ref = shape_set(n_cells, n_angles)
    rec, curve = run_device(ctx, imgs, ref, offset=offset)
    assert_records(rec, curve, expected(imgs, ref, ("set", (n_cells, n_angles))))
    ctx.close()


def test_seventy_images_cross_the_chunk():
    n, n_cells, n_angles = 70, 64, 37
    ctx = conv_ctx(n_cells, n_angles)
    imgs, ref = image_set(n, n_cells, n_angles, seed=70)
    imgs[65] = np.roll(ref, 11, axis=1)
    want = expected(imgs, ref, "seventy")
    rec, curve = run_device(ctx, imgs, ref)
    assert_records(rec, curve, want)
    assert rec["shift"][65] == n_angles - 11 and rec["sse"][65] == 0
    h_rec, h_curve = ctx.align_images(imgs, ref, want_curve=True)
    assert h_rec.tobytes() == rec.tobytes() and np.array_equal(h_curve, curve)
    ctx.close()


def test_simulated_batch():
    """a small scene (config 2's, 2 passes, 200 cells of half a metre, noise off): the records of rr_simulate_batch_align are
    those of rr_align_images on the images rr_simulate_batch_device renders for the same poses"""
    scene = scenes.config_scene(2)
    cfg = params.kaist_preset(n_reflections=2, n_samples=50, ambient_noise=0, n_cells=200, resolution=0.5)
    ctx = native.Context(0)
    ctx.set_mesh(scene["verts"], scene["faces"], scene["face_object_id"])
    ctx.set_materials(materials_for(scene), scene["object_materials"], 0)
    ctx.set_config(cfg, 400)
    ctx.set_beam_samples(golden_beams(50))
    poses = np.asarray(scenes.trajectory(3, scene["name"]), np.float32).reshape(3, 7)
    d_imgs = torch.zeros((3, 200, 400), dtype=torch.uint8, device=DEV)
    ctx.simulate_batch_device(poses, d_imgs.data_ptr())
    ctx.synchronize()
    imgs = d_imgs.cpu().numpy()
    assert imgs[1].any()
    ref = np.roll(imgs[1], 37, axis=1)
    out, rec, curve = ctx.simulate_batch_align(poses, ref, want_images=True, want_curve=True)
    assert np.array_equal(out, imgs)
    h_rec, h_curve = ctx.align_images(imgs, ref, want_curve=True)
    assert rec.tobytes() == h_rec.tobytes() and np.array_equal(curve, h_curve)
    assert_records(rec, curve, [A.align(im, ref) for im in imgs])
    # x = pose 1's image, r = x rolled by 37: r[c][a + 37] = x[c][a]
    assert rec["shift"][1] == 37 and rec["sse"][1] == 0
    ref = np.roll(imgs[1], -37, axis=1)
    none, rec, no_curve = ctx.simulate_batch_align(poses, ref, 10, 200)
    assert none is None and no_curve is None
    assert rec["shift"][1] == 400 - 37 and rec["sse"][1] == 0 and np.isinf(rec["psnr"][1])
    assert rec.tobytes() == ctx.align_images(imgs, ref, 10, 200).tobytes()
    ctx.close()


def test_python_facade_align_images():
    from radarays_ros_amd import radar
    s = scenes.box12()
    r = radar.RadarHIP(s["verts"], s["faces"], s["face_object_id"])
    r.loadParams(params.kaist_materials(), s["object_materials"], 0)
    r.updateDynCfg(params.kaist_preset(n_reflections=1, ambient_noise=0, n_cells=100))
    imgs, ref = shape_set(100, 400)
    rec, curve = r.alignImages(list(imgs), ref, want_curve=True)
    assert_records(rec, curve, expected(imgs, ref, ("set", (100, 400))))
    assert r.alignImages(imgs[0], ref, 3, 90)["shift"][0] == 400 - 11


def test_refusals_are_negative_with_a_message_and_write_nothing():
    ctx = conv_ctx(64, 16)
    L, h = ctx._L, ctx._h
    imgs, ref = image_set(2, 64, 16, seed=3)
    d_imgs, d_ref = torch.from_numpy(imgs).to(DEV), torch.from_numpy(ref).to(DEV)
    d_curve = torch.full((2, 16), POISON, dtype=torch.int64, device=DEV)
    out = np.full(2 * REC_BYTES, 0x5A, np.uint8)
    h_curve = np.full((2, 16), POISON, np.int64)
    o, i, r, dc = out.ctypes.data, d_imgs.data_ptr(), d_ref.data_ptr(), d_curve.data_ptr()
    pose = np.zeros(7, np.float32)

    def refused(rc, text):
        assert rc == -3, rc
        assert text in L.rr_last_error(h), L.rr_last_error(h)
    for args in ((None, 2, r, 0, 64, o, dc), (i, 2, None, 0, 64, o, dc), (i, 2, r, 0, 64, None, dc)):
        refused(L.rr_align_images_device(h, *args, None), b"rr_align_images_device: null buffer")
    for n in (0, 65536, -1):
        refused(L.rr_align_images_device(h, i, n, r, 0, 64, o, dc, None), b"n_images")
    for cb, ce in ((-1, 64), (0, 65), (5, 5), (6, 5), (64, 64), (0, 0)):
        refused(L.rr_align_images_device(h, i, 2, r, cb, ce, o, dc, None), b"cell window")
        refused(L.rr_align_images(h, imgs.ctypes.data, 2, ref.ctypes.data, cb, ce, o, h_curve.ctypes.data), b"rr_align_images: the cell window")
        refused(L.rr_simulate_batch_align(h, pose.ctypes.data, 1, ref.ctypes.data, cb, ce, None, o, h_curve.ctypes.data), b"rr_simulate_batch_align: the cell window")
    refused(L.rr_align_images(h, imgs.ctypes.data, 2, None, 0, 64, o, h_curve.ctypes.data), b"null buffer")
    refused(L.rr_align_images(h, None, 2, ref.ctypes.data, 0, 64, o, h_curve.ctypes.data), b"null buffer")
    refused(L.rr_align_images(h, imgs.ctypes.data, 0, ref.ctypes.data, 0, 64, o, h_curve.ctypes.data), b"n_images")
    refused(L.rr_simulate_batch_align(h, pose.ctypes.data, 1, None, 0, 64, None, o, None), b"null buffer")
    refused(L.rr_simulate_batch_align(h, pose.ctypes.data, 1, ref.ctypes.data, 0, 64, None, None, None), b"null buffer")
    for n in (0, 65):
        refused(L.rr_simulate_batch_align(h, pose.ctypes.data, n, ref.ctypes.data, 0, 64, None, o, None), b"n_images must be 1..64")
    # a window of more than 2^23 pixels: 8185 x 1025 = 8,389,625 (8184 x 1025 = 8,388,600 would pass)
    big = conv_ctx(8192, 1025)
    for cb, ce in ((0, 8185), (7, 8192), (0, 8192)):
        assert big._L.rr_align_images_device(big._h, i, 1, r, cb, ce, o, None, None) == -3
        assert b"2^23" in big._L.rr_last_error(big._h)
    # a context without a config; one with a config and no mesh cannot simulate
    bare = native.Context(0)
    assert bare._L.rr_align_images_device(bare._h, i, 2, r, 0, 64, o, dc, None) == -2
    assert bare._L.rr_align_images(bare._h, imgs.ctypes.data, 2, ref.ctypes.data, 0, 64, o, None) == -2
    assert b"rr_set_config" in bare._L.rr_last_error(bare._h)
    assert L.rr_simulate_batch_align(h, pose.ctypes.data, 1, ref.ctypes.data, 0, 64, None, o, h_curve.ctypes.data) == -2
    torch.cuda.synchronize()
    assert np.all(out == 0x5A) and np.all(h_curve == POISON) and bool((d_curve == POISON).all())
    ok = ctx.align_images_device(i, 2, r)                                 # the same buffers are fine
    assert ok["shift"][1] == 0 and ok["sse"][1] == 0                      # image 1 is the reference itself
    for c in (ctx, big, bare):
        c.close()
