"""Translation registration on the GPU (rr_shift.hip: rr_shift_images_device, rr_shift_images, rr_simulate_batch_shift) against
the numpy restatement of its definition (tests/shift_ref.py).

Bounds.  The two surfaces, dy, dx, n_best, xcorr, sse, the neighbours' sse and the four sums are integers and compared bit for
bit; so are psnr, sub_dy and sub_dx, which the host forms from exact integers by the same f64 operations as the restatement.
ncc within 1 ulp: its three inputs are exact integers, and sqrt and the divide are correctly rounded on both sides, but the GPU
is free to fuse nothing or something else than numpy around them.
The simulated case is held to one pixel on each axis: half a pixel of resampling per image, not to be widened."""
import ctypes as C

import numpy as np
import pytest

import shift_ref as R
from common import golden_beams
from radarays_ros_amd import native, params
from test_gpu_metrics import dark
from test_shift_host import SIM, sim_poses

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
POISON = 0x5A5A5A5A5A5A5A5A
INT_FIELDS = ("dy", "dx", "n_best", "xcorr", "sse", "sum_x", "sum_xx", "sum_r", "sum_rr")
REC_BYTES = native.SHIFT_DTYPE.itemsize


def run_device(ctx, imgs, ref, S, offset=0, want_surfaces=True):
    """the images (and the reference) at `offset` bytes past an aligned device allocation, the surface buffers poisoned ->
    (records, xcorr int64 [n][D][D], sse uint64 [n][D][D])"""
    n, H, W = imgs.shape
    D = 2 * S + 1
    buf = torch.zeros(imgs.size + offset + 16, dtype=torch.uint8, device=DEV)
    buf[offset:offset + imgs.size] = torch.from_numpy(imgs.ravel()).to(DEV)
    rbuf = torch.zeros(ref.size + offset + 16, dtype=torch.uint8, device=DEV)
    rbuf[offset:offset + ref.size] = torch.from_numpy(ref.ravel()).to(DEV)
    d_xc = torch.full((n, D, D), POISON, dtype=torch.int64, device=DEV) if want_surfaces else None
    d_sse = torch.full((n, D, D), POISON, dtype=torch.int64, device=DEV) if want_surfaces else None
    torch.cuda.synchronize()
    rec = ctx.shift_images_device(buf.data_ptr() + offset, n, rbuf.data_ptr() + offset, H, W, S,
                                  None if d_xc is None else d_xc.data_ptr(), None if d_sse is None else d_sse.data_ptr())
    if not want_surfaces:
        return rec, None, None
    return rec, d_xc.cpu().numpy(), d_sse.cpu().numpy().view(np.uint64)


_WANT = {}


def expected(imgs, ref, S, key):
    """the restatement's records (with their surfaces), computed once per image set"""
    if key not in _WANT:
        box = R.box_sums(ref, S)
        _WANT[key] = [R.shift(im, ref, S, box=box) for im in imgs]
    return _WANT[key]


def assert_records(rec, xc, sse, want):
    assert len(rec) == len(want)
    for k, w in enumerate(want):
        r = rec[k]
        print("image %d: (dy, dx) (%d, %d) want (%d, %d) n_best %d xcorr %d sse %d psnr %r (want %r) ncc %.17g (want %.17g) sub (%r, %r) want (%r, %r)" % (
            k, r["dy"], r["dx"], w["dy"], w["dx"], r["n_best"], r["xcorr"], r["sse"], float(r["psnr"]), w["psnr"], r["ncc"], w["ncc"],
            float(r["sub_dy"]), float(r["sub_dx"]), w["sub_dy"], w["sub_dx"]))
        if xc is not None:
            assert np.array_equal(xc[k], w["xcorr_surface"]), (k, np.argwhere(xc[k] != w["xcorr_surface"])[:8])
        if sse is not None:
            assert np.array_equal(sse[k], w["sse_surface"]), (k, np.argwhere(sse[k] != w["sse_surface"])[:8])
        for f in INT_FIELDS:
            assert int(r[f]) == w[f], (k, f, int(r[f]), w[f])
        assert [int(v) for v in r["sse_nb"]] == w["sse_nb"], (k, r["sse_nb"], w["sse_nb"])
        assert r["reserved_"] == 0
        assert abs(r["ncc"] - w["ncc"]) <= np.spacing(abs(w["ncc"])), (k, r["ncc"], w["ncc"])
        for f in ("psnr", "sub_dy", "sub_dx"):
            assert float(r[f]) == w[f], (k, f, float(r[f]), w[f])


def shape_set(H, W, S):
    """three images: the reference moved so that it is found at (p, q) = (min(S, 2), -min(S, 3)), a 30 % corrupted copy of the
    reference, other noise"""
    rs = np.random.RandomState(H + W + S)
    ref = dark((H, W), rs)
    p, q = min(S, 2), -min(S, 3)
    moved = np.roll(ref, (-p, -q), axis=(0, 1))          # moved[i][j] = ref[i + p][j + q] wherever T reaches
    noisy = ref.copy()
    hit = rs.rand(H, W) < 0.3
    noisy[hit] = rs.randint(0, 256, int(hit.sum()))
    return np.stack([moved, noisy, dark((H, W), rs)]), ref, (p, q)


SHAPES = [(40, 37, 3), (100, 70, 32), (150, 200, 64), (1200, 48, 4), (512, 512, 32)]


@pytest.mark.parametrize("shape", SHAPES, ids=["40x37_S3_one_ragged_tile", "100x70_S32_three_band_tiles", "150x200_S64_five_band_tiles",
                                              "1200x48_S4_two_k_chunks", "512x512_S32_workload_class"])
def test_surfaces_and_records_match_the_restatement(shape):
    H, W, S = shape
    ctx = native.Context(0)                              # no config, no mesh
    imgs, ref, (p, q) = shape_set(H, W, S)
    want = expected(imgs, ref, S, ("set", shape))
    rec, xc, sse = run_device(ctx, imgs, ref, S)
    assert_records(rec, xc, sse, want)
    r0 = rec[0]
    assert (r0["dy"], r0["dx"]) == (p, q) and r0["sse"] == 0 and np.isinf(r0["psnr"]) and r0["psnr"] > 0 and r0["n_best"] == 1
    assert abs(r0["ncc"] - 1.0) <= np.spacing(1.0) and abs(r0["sub_dy"]) <= 0.5 and abs(r0["sub_dx"]) <= 0.5
    # two identical calls return identical bytes
    again, xc2, sse2 = run_device(ctx, imgs, ref, S)
    assert rec.tobytes() == again.tobytes() and xc.tobytes() == xc2.tobytes() and sse.tobytes() == sse2.tobytes()
    # without surface buffers, and the host form
    bare, _, _ = run_device(ctx, imgs, ref, S, want_surfaces=False)
    assert bare.tobytes() == rec.tobytes()
    h_rec, h_xc, h_sse = ctx.shift_images(imgs, ref, S, want_surfaces=True)
    assert h_rec.tobytes() == rec.tobytes() and np.array_equal(h_xc, xc) and np.array_equal(h_sse, sse)
    assert ctx.shift_images(imgs, ref, S).tobytes() == rec.tobytes()
    ctx.close()


SINGLE = [(7, 5), (7, -5), (-7, 5), (-7, -5), (2, -9), (0, 0)]


@pytest.mark.parametrize("shape", [(40, 37, 3), (100, 70, 32)], ids=["40x37_S3", "100x70_S32"])
def test_single_pixels(shape):
    """x has one pixel of value 3 at (i0, j0), r one of value 5 at (i1, j1): 15 at (i1 - i0, j1 - j0) and 0 elsewhere.  All four
    sign combinations, and (2, -9) with |dy| != |dx|: a swapped row and column cannot hide"""
    H, W, S = shape
    ctx = native.Context(0)
    i0, j0 = H // 2, W // 2 - 1
    cases = [(dy, dx) for dy, dx in SINGLE if abs(dy) <= S and abs(dx) <= S] if S >= 9 else [(2, 3), (2, -3), (-2, 3), (-2, -3), (1, -3), (0, 0)]
    x = np.zeros((len(cases), H, W), np.uint8)
    x[:, i0, j0] = 3
    for k, (dy, dx) in enumerate(cases):
        r = np.zeros((H, W), np.uint8)
        r[i0 + dy, j0 + dx] = 5
        rec, xc, sse = run_device(ctx, x[k:k + 1], r, S)
        want = np.zeros((2 * S + 1, 2 * S + 1), np.int64)
        want[dy + S, dx + S] = 15
        assert np.array_equal(xc[0], want), (dy, dx, np.argwhere(xc[0]))
        assert (rec["dy"][0], rec["dx"][0]) == (dy, dx) and rec["n_best"][0] == 1 and rec["xcorr"][0] == 15 and rec["sse"][0] == 9 + 25 - 30
        assert (rec["sum_x"][0], rec["sum_xx"][0], rec["sum_r"][0], rec["sum_rr"][0]) == (3, 9, 5, 25)
        assert_records(rec, xc, sse, [R.shift(x[k], r, S)])
    ctx.close()


def test_constant_images():
    """all-0 against all-0 and all-255 against all-255 at (1200, 96, 32): the largest signed magnitudes, over two K-chunks; every
    shift ties, the tie goes to index 0"""
    H, W, S = 1200, 96, 32
    D, n_px = 2 * S + 1, (H - 2 * S) * (W - 2 * S)
    ctx = native.Context(0)
    zero, full = np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8)
    rec, xc, sse = run_device(ctx, np.stack([zero, zero]), zero, S)
    assert not xc.any() and not sse.any()
    for f, v in (("dy", -S), ("dx", -S), ("n_best", D * D), ("xcorr", 0), ("sse", 0), ("sum_x", 0), ("sum_xx", 0), ("sum_r", 0), ("sum_rr", 0)):
        assert np.all(rec[f] == v), (f, rec[f])
    assert np.all(rec["ncc"] == 0.0) and np.all(np.isinf(rec["psnr"])) and np.all(rec["psnr"] > 0)
    assert np.all(rec["sub_dy"] == 0.0) and np.all(rec["sub_dx"] == 0.0)
    rec, xc, sse = run_device(ctx, np.stack([full, zero]), full, S)
    assert np.all(xc[0] == 255 * 255 * n_px) and not xc[1].any() and not sse[0].any() and np.all(sse[1] == 255 * 255 * n_px)
    assert (rec["dy"][0], rec["dx"][0]) == (-S, -S) and rec["n_best"][0] == D * D and rec["xcorr"][0] == 255 * 255 * n_px and rec["sse"][0] == 0
    assert rec["ncc"][0] == 0.0 and rec["sum_x"][0] == 255 * n_px and rec["sum_rr"][0] == 255 * 255 * n_px
    assert rec["n_best"][1] == D * D and rec["sse"][1] == 255 * 255 * n_px
    assert [int(v) for v in rec["sse_nb"][0]] == [R.U64_MAX, 0, R.U64_MAX, 0]
    ctx.close()


@pytest.mark.parametrize("offset", [1, 3])
def test_images_at_odd_byte_offsets(offset):
    H, W, S = 100, 70, 32
    ctx = native.Context(0)
    imgs, ref, _ = shape_set(H, W, S)
    rec, xc, sse = run_device(ctx, imgs, ref, S, offset=offset)
    assert_records(rec, xc, sse, expected(imgs, ref, S, ("set", (H, W, S))))
    ctx.close()


def test_seventy_images_cross_the_chunk():
    n, H, W, S = 70, 40, 37, 3
    ctx = native.Context(0)
    rs = np.random.RandomState(70)
    ref = dark((H, W), rs)
    imgs = np.stack([dark((H, W), rs) for _ in range(n)])
    imgs[65] = np.roll(ref, (1, -2), axis=(0, 1))        # found at (-1, 2)
    want = expected(imgs, ref, S, "seventy")
    rec, xc, sse = run_device(ctx, imgs, ref, S)
    assert_records(rec, xc, sse, want)
    assert (rec["dy"][65], rec["dx"][65]) == (-1, 2) and rec["sse"][65] == 0
    h_rec, h_xc, h_sse = ctx.shift_images(imgs, ref, S, want_surfaces=True)
    assert h_rec.tobytes() == rec.tobytes() and np.array_equal(h_xc, xc) and np.array_equal(h_sse, sse)
    ctx.close()


def sim_ctx():
    scene = SIM["scene"]()
    ctx = native.Context(0)
    ctx.set_mesh(scene["verts"], scene["faces"], scene["face_object_id"])
    ctx.set_materials(params.kaist_materials(), scene["object_materials"], 0)
    ctx.set_config(SIM["cfg"](), 400)
    ctx.set_beam_samples(golden_beams(SIM["n_samples"]))
    return ctx


def test_simulated_translation_is_found_within_a_pixel():
    """one small scene (tests/test_shift_host.py fixes it, and the two poses, on the CPU), noise off: the image rendered at pose
    x against the polar image rendered at pose r, of equal yaw and displaced by (+6, -4) pixels' worth of metres"""
    ctx = sim_ctx()
    pose_x, pose_r = sim_poses()
    W, ps, S = SIM["width"], SIM["pixel_size"], SIM["max_shift"]
    d_img = torch.zeros((1, SIM["n_cells"], 400), dtype=torch.uint8, device=DEV)
    ctx.simulate_batch_device(pose_r[None], d_img.data_ptr())
    ctx.synchronize()
    ref_polar = d_img.cpu().numpy()[0]
    assert ref_polar.any()
    cart, rec, xc = ctx.simulate_batch_shift(np.stack([pose_x, pose_r]), ref_polar, W, ps, S, want_images=True, want_xcorr=True)
    print("simulated: (dy, dx) = (%d, %d) sub (%.3f, %.3f) sse %d ncc %.6f; the reference pose itself: (%d, %d) sse %d" % (
        rec["dy"][0], rec["dx"][0], rec["sub_dy"][0], rec["sub_dx"][0], rec["sse"][0], rec["ncc"][0], rec["dy"][1], rec["dx"][1], rec["sse"][1]))
    assert abs(int(rec["dy"][0]) - 6) <= 1 and abs(int(rec["dx"][0]) + 4) <= 1
    assert (rec["dy"][1], rec["dx"][1]) == (0, 0) and rec["sse"][1] == 0          # the reference's own pose gives the reference's own image
    # the records are those of rr_shift_images on the Cartesian images the call hands out, against the Cartesian reference
    ref_cart = ctx.polar_to_cartesian(ref_polar, W, ps)[0]
    assert np.array_equal(cart[1], ref_cart)
    h_rec, h_xc, _ = ctx.shift_images(cart, ref_cart, S, want_surfaces=True)
    assert h_rec.tobytes() == rec.tobytes() and np.array_equal(h_xc, xc)
    assert_records(rec, xc, None, [R.shift(im, ref_cart, S) for im in cart])
    none, rec2, no_xc = ctx.simulate_batch_shift(np.stack([pose_x, pose_r]), ref_polar, W, ps, S)
    assert none is None and no_xc is None and rec2.tobytes() == rec.tobytes()
    ctx.close()


def test_python_facade_register_translation_and_pose():
    from radarays_ros_amd import radar
    scene = SIM["scene"]()
    r = radar.RadarHIP(scene["verts"], scene["faces"], scene["face_object_id"])
    r.loadParams(params.kaist_materials(), scene["object_materials"], 0)
    r.updateDynCfg(SIM["cfg"]())
    r.setBeamSamples(golden_beams(SIM["n_samples"]))
    pose_x, pose_r = sim_poses()
    W, ps, S = SIM["width"], SIM["pixel_size"], SIM["max_shift"]
    imgs = r.simulateBatch(np.stack([pose_x, pose_r]))
    rec, corr = r.registerTranslation(imgs[0], imgs[1], W, ps, S)
    ctx = r.context
    cart = ctx.polar_to_cartesian(np.stack([imgs[0].data, imgs[1].data]), W, ps)
    assert_records(rec, None, None, [R.shift(cart[0], cart[1], S)])
    assert abs(int(rec["dy"][0]) - 6) <= 1 and abs(int(rec["dx"][0]) + 4) <= 1
    assert corr.shape == (1, 2) and corr[0, 0] == (rec["dy"][0] + rec["sub_dy"][0]) * ps and corr[0, 1] == (rec["dx"][0] + rec["sub_dx"][0]) * ps
    # the corrected pose lies within a pixel of the pose the real image was taken at, on both axes, and keeps its yaw
    fixed, yaw_rec, shift_rec = r.registerPose(pose_x[None], imgs[1], W, ps, S)
    print("registerPose:", pose_x, "->", fixed[0], "wanted", pose_r, "yaw shift", yaw_rec["shift"][0])
    assert yaw_rec["shift"][0] == 0
    assert np.all(np.abs(fixed[0, 4:6] - pose_r[4:6]) <= ps * np.sqrt(2.0) + 1e-6) and np.array_equal(fixed[0, :4], pose_x[:4])
    assert fixed[0, 6] == pose_x[6]


def test_refusals_are_negative_with_a_message_and_write_nothing():
    ctx = native.Context(0)
    L, h = ctx._L, ctx._h
    H, W, S = 40, 37, 3
    D = 2 * S + 1
    rs = np.random.RandomState(3)
    imgs, ref = np.stack([dark((H, W), rs) for _ in range(2)]), dark((H, W), rs)
    d_imgs, d_ref = torch.from_numpy(imgs).to(DEV), torch.from_numpy(ref).to(DEV)
    d_xc = torch.full((2, D, D), POISON, dtype=torch.int64, device=DEV)
    d_sse = torch.full((2, D, D), POISON, dtype=torch.int64, device=DEV)
    out = np.full(2 * REC_BYTES, 0x5A, np.uint8)
    h_xc, h_sse = np.full((2, D, D), POISON, np.int64), np.full((2, D, D), POISON, np.int64)
    o, i, r, dx, ds = out.ctypes.data, d_imgs.data_ptr(), d_ref.data_ptr(), d_xc.data_ptr(), d_sse.data_ptr()
    hi, hr = imgs.ctypes.data, ref.ctypes.data

    def refused(rc, text):
        assert rc == -3, rc
        assert text in L.rr_last_error(h), L.rr_last_error(h)
    for a in ((None, 2, r, H, W, S, o), (i, 2, None, H, W, S, o), (i, 2, r, H, W, S, None)):
        refused(L.rr_shift_images_device(h, *a, dx, ds, None), b"rr_shift_images_device: null buffer")
    for n in (0, 65536, -1):
        refused(L.rr_shift_images_device(h, i, n, r, H, W, S, o, dx, ds, None), b"n_images")
        refused(L.rr_shift_images(h, hi, n, hr, H, W, S, o, h_xc.ctypes.data, h_sse.ctypes.data), b"rr_shift_images: n_images")
    for hh, ww, ss, text in ((0, W, 0, b"height and width"), (H, 8193, S, b"height and width"), (H, W, -1, b"max_shift"), (H, W, 65, b"max_shift"),
                             (6, W, 3, b"no template window"), (H, 6, 3, b"no template window"), (H, W, 19, b"no template window"),
                             (4096, 2049, 0, b"2^23")):
        refused(L.rr_shift_images_device(h, i, 2, r, hh, ww, ss, o, dx, ds, None), text)
        refused(L.rr_shift_images(h, hi, 2, hr, hh, ww, ss, o, h_xc.ctypes.data, h_sse.ctypes.data), text)
    refused(L.rr_shift_images(h, None, 2, hr, H, W, S, o, None, None), b"null buffer")
    refused(L.rr_shift_images(h, hi, 2, None, H, W, S, o, None, None), b"null buffer")
    refused(L.rr_shift_images(h, hi, 2, hr, H, W, S, None, None, None), b"null buffer")
    # rr_simulate_batch_shift: a context without a config is -2; with one, its own refusals come before anything is simulated
    pose = np.zeros(7, np.float32)
    cc = native.cartesian_config(64, 0.5)
    polar = np.zeros((64, 16), np.uint8)
    assert L.rr_simulate_batch_shift(h, pose.ctypes.data, 1, polar.ctypes.data, C.byref(cc), 3, None, o, None) == -2
    assert b"rr_set_config" in L.rr_last_error(h)
    ctx.set_config(params.kaist_preset(n_cells=64), 16)
    refused(L.rr_simulate_batch_shift(h, pose.ctypes.data, 1, None, C.byref(cc), 3, None, o, None), b"rr_simulate_batch_shift: null")
    refused(L.rr_simulate_batch_shift(h, pose.ctypes.data, 1, polar.ctypes.data, None, 3, None, o, None), b"null config")
    refused(L.rr_simulate_batch_shift(h, pose.ctypes.data, 1, polar.ctypes.data, C.byref(cc), 3, None, None, None), b"null")
    for n in (0, 65):
        refused(L.rr_simulate_batch_shift(h, pose.ctypes.data, n, polar.ctypes.data, C.byref(cc), 3, None, o, h_xc.ctypes.data), b"n_images must be 1..64")
    for ss, text in ((-1, b"max_shift"), (65, b"max_shift"), (32, b"no template window")):
        refused(L.rr_simulate_batch_shift(h, pose.ctypes.data, 1, polar.ctypes.data, C.byref(cc), ss, None, o, h_xc.ctypes.data), text)
    assert L.rr_simulate_batch_shift(h, pose.ctypes.data, 1, polar.ctypes.data, C.byref(cc), 3, None, o, h_xc.ctypes.data) == -2      # no mesh
    torch.cuda.synchronize()
    assert np.all(out == 0x5A) and np.all(h_xc == POISON) and np.all(h_sse == POISON)
    assert bool((d_xc == POISON).all()) and bool((d_sse == POISON).all())
    ok = ctx.shift_images_device(i, 2, r, H, W, S)                        # the same buffers are fine
    assert ok.tobytes() == ctx.shift_images(imgs, ref, S).tobytes()
    ctx.close()
