"""Real-to-sim image metrics on the GPU (rr_metrics.hip: rr_compare_images_device, rr_compare_images,
rr_simulate_param_sets_metrics) against the numpy / scipy restatement of their definitions (tests/metrics_ref.py).

Bounds.  The joint histogram, SSE and PSNR are compared bit for bit.  SSIM within 1e-9 absolute: the window sums are exact,
a pixel's S carries about 1e-13 of f64 rounding, and any summation order of N <= 1.4e6 terms in [-1, 1] stays below
N * 2^-53 = 1.5e-10.  The entropies and what is formed from them within 1e-9 absolute: at most 65,536 terms, each a few ulps
of the GPU's f64 log, entropies below ln(65,536) = 11.1 nats."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import metrics_ref as M
from common import golden_beams, materials_for, mats_tuple
from radarays_ros_amd import native, params, scenes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9
INFO_KEYS = ("hx", "hy", "hxy", "mi", "nmi", "voi")
ALL = native.METRIC_ALL


def conv_ctx(n_cells, n_angles):
    """a context with a config and no mesh: what a caller comparing real images has"""
    c = native.Context(0)
    c.set_config(params.kaist_preset(n_cells=n_cells), n_angles)
    return c


def dark(shape, rs):
    """dark noise with sparse strong peaks (as in test_gpu_detect.py)"""
    img = rs.randint(0, 30, shape).astype(np.uint8)
    peaks = rs.rand(*shape) < 0.02
    img[peaks] = rs.randint(80, 256, int(peaks.sum()))
    return img


def image_set(n, n_cells, n_angles, seed):
    """reference = dark noise with peaks; images cycle through a 30 % corrupted copy, the reference itself, all-zero,
    other noise, all-255"""
    rs = np.random.RandomState(seed)
    ref = dark((n_cells, n_angles), rs)
    imgs = np.empty((n, n_cells, n_angles), np.uint8)
    for k in range(n):
        if k % 5 == 0:
            imgs[k] = ref
            hit = rs.rand(n_cells, n_angles) < 0.3
            imgs[k][hit] = rs.randint(0, 256, int(hit.sum()))
        elif k % 5 == 1:
            imgs[k] = ref
        elif k % 5 == 2:
            imgs[k] = 0
        elif k % 5 == 3:
            imgs[k] = dark((n_cells, n_angles), rs)
        else:
            imgs[k] = 255
    return imgs, ref


_WANT = {}


def expected(imgs, ref, win, key):
    """the restatement's records and histograms, computed once per image set and window"""
    if key not in _WANT:
        out = []
        for im in imgs:
            H = M.joint_histogram(im, ref)
            sse, psnr = M.psnr(im, ref)
            out.append(dict(M.info(H), H=H, sse=sse, psnr=psnr, ssim=M.ssim(im, ref, win)))
        _WANT[key] = out
    return _WANT[key]


def assert_records(rec, hist, want, n_px, which=ALL):
    for k, w in enumerate(want):
        r = rec[k]
        print("image %d: ssim %.12f (want %.12f, diff %.2e) hxy %.12f (diff %.2e) mi diff %.2e nmi diff %.2e" % (
            k, r["ssim"], w["ssim"], abs(r["ssim"] - w["ssim"]), r["hxy"], abs(r["hxy"] - w["hxy"]), abs(r["mi"] - w["mi"]),
            abs(r["nmi"] - w["nmi"])))
        if which & native.METRIC_INFO:
            if hist is not None:
                assert np.array_equal(hist[k], w["H"]), k
                assert int(hist[k].sum(dtype=np.uint64)) == n_px
            for key in INFO_KEYS:
                assert abs(r[key] - w[key]) <= TOL, (k, key, r[key], w[key])
        else:
            assert all(r[key] == 0.0 for key in INFO_KEYS), k
        if which & native.METRIC_SSIM:
            assert abs(r["ssim"] - w["ssim"]) <= TOL, (k, r["ssim"], w["ssim"])
        else:
            assert r["ssim"] == 0.0
        if which & native.METRIC_PSNR:
            assert int(r["sse"]) == w["sse"], k
            assert (np.isinf(r["psnr"]) and r["psnr"] > 0 and w["sse"] == 0) or abs(r["psnr"] - w["psnr"]) <= TOL, (k, r["psnr"])
        else:
            assert r["psnr"] == 0.0 and r["sse"] == 0


def run_device(ctx, imgs, ref, which=ALL, win=7, offset=0, want_hist=True):
    """the images at `offset` bytes past an aligned device allocation -> (records, histograms, psnr, sse of rr_score_images_device)"""
    n = len(imgs)
    buf = torch.zeros(imgs.size + offset + 16, dtype=torch.uint8, device=DEV)
    buf[offset:offset + imgs.size] = torch.from_numpy(imgs.ravel()).to(DEV)
    d_ref = torch.from_numpy(ref).to(DEV)
    d_hist = torch.full((n, 256, 256), 0x5A5A5A5A, dtype=torch.int32, device=DEV) if want_hist else None
    torch.cuda.synchronize()
    ptr = buf.data_ptr() + offset
    rec = ctx.compare_images_device(ptr, n, d_ref.data_ptr(), which, win, None if d_hist is None else d_hist.data_ptr())
    psnr, sse = ctx.score_images_device(ptr, n, d_ref.data_ptr(), want_sse=True)
    hist = None if d_hist is None else d_hist.cpu().numpy().view(np.uint32)
    return rec, hist, psnr, sse


SHAPES = [(3, 7, 7, 0), (4, 100, 37, 0), (16, 200, 400, 0), (2, 3424, 400, 0), (70, 64, 64, 0), (5, 100, 400, 1)]


@pytest.mark.parametrize("shape", SHAPES, ids=["3x7x7_one_window", "4x100x37_no_16B_rows", "16x200x400", "2x3424x400",
                                               "70x64x64_two_chunks", "5x100x400_base_plus_1"])
def test_metrics_match_the_restatement(shape):
    n, n_cells, n_angles, offset = shape
    ctx = conv_ctx(n_cells, n_angles)
    imgs, ref = image_set(n, n_cells, n_angles, seed=n_cells + n_angles)
    want = expected(imgs, ref, 7, ("set", shape[:3]))
    rec, hist, psnr, sse = run_device(ctx, imgs, ref, offset=offset)
    assert_records(rec, hist, want, n_cells * n_angles)
    # sse and psnr: the bits of rr_score_images_device on the same buffers
    assert np.array_equal(rec["sse"], sse) and np.array_equal(rec["psnr"].view(np.uint64), psnr.view(np.uint64))
    if n > 1:           # image 1 is the reference itself
        assert rec["ssim"][1] == 1.0 and np.isinf(rec["psnr"][1]) and rec["psnr"][1] > 0 and rec["mi"][1] == rec["hx"][1]
        assert rec["hx"][1] == rec["hy"][1] == rec["hxy"][1] and rec["voi"][1] == 0.0
    # two identical calls return identical bits
    again, hist2, _, _ = run_device(ctx, imgs, ref, offset=offset)
    assert rec.tobytes() == again.tobytes() and np.array_equal(hist, hist2)
    # the host form equals the device form
    h_rec, h_hist = ctx.compare_images(imgs, ref, want_hist=True)
    assert h_rec.tobytes() == rec.tobytes() and np.array_equal(h_hist, hist)
    ctx.close()


def test_constant_images():
    """all-zero against all-255: one bin holds everything, hxy = 0 and nmi = 1; all-zero against noise; and 1,369,600 pixels
    in ONE bin (all-zero against an all-zero reference at full size): a 16-bit private count must not wrap"""
    n_cells, n_angles = 100, 37
    ctx = conv_ctx(n_cells, n_angles)
    rs = np.random.RandomState(8)
    ref = np.full((n_cells, n_angles), 255, np.uint8)
    imgs = np.stack([np.zeros_like(ref), ref, dark(ref.shape, rs)])
    rec, hist, _, _ = run_device(ctx, imgs, ref)
    assert_records(rec, hist, expected(imgs, ref, 7, "const255"), n_cells * n_angles)
    assert hist[0][0, 255] == n_cells * n_angles
    for k in (0, 1):
        assert rec["hxy"][k] == 0.0 and rec["nmi"][k] == 1.0 and rec["mi"][k] == 0.0 and rec["voi"][k] == 0.0
    assert rec["hy"][2] == 0.0 and rec["hxy"][2] > 0 and abs(rec["nmi"][2] - 1.0) <= TOL              # hx + hy == hxy
    ctx.close()
    n_cells, n_angles = 3424, 400
    ctx = conv_ctx(n_cells, n_angles)
    ref = np.zeros((n_cells, n_angles), np.uint8)
    imgs = np.stack([ref, dark(ref.shape, rs)])
    rec, hist, _, _ = run_device(ctx, imgs, ref)
    assert hist[0][0, 0] == 1369600 and int(hist[0].sum(dtype=np.uint64)) == 1369600
    assert_records(rec, hist, expected(imgs, ref, 7, "const0"), n_cells * n_angles)
    assert rec["ssim"][0] == 1.0 and rec["hxy"][0] == 0.0 and rec["nmi"][0] == 1.0
    ctx.close()


@pytest.mark.parametrize("win", [3, 11, 15])
def test_other_window_sizes(win):
    n, n_cells, n_angles = 4, 100, 37
    ctx = conv_ctx(n_cells, n_angles)
    imgs, ref = image_set(n, n_cells, n_angles, seed=n_cells + n_angles)
    rec, hist, _, _ = run_device(ctx, imgs, ref, win=win)
    assert_records(rec, hist, expected(imgs, ref, win, ("win", win)), n_cells * n_angles)
    assert rec["ssim"][1] == 1.0
    ctx.close()


def test_masks_leave_the_other_fields_zero():
    n, n_cells, n_angles = 4, 100, 37
    ctx = conv_ctx(n_cells, n_angles)
    imgs, ref = image_set(n, n_cells, n_angles, seed=n_cells + n_angles)
    want = expected(imgs, ref, 7, ("set", (n, n_cells, n_angles)))
    full, _, _, _ = run_device(ctx, imgs, ref)
    for which in (native.METRIC_SSIM, native.METRIC_PSNR, native.METRIC_INFO, native.METRIC_PSNR | native.METRIC_INFO):
        rec, _, _, _ = run_device(ctx, imgs, ref, which=which, want_hist=bool(which & native.METRIC_INFO))
        assert_records(rec, None, want, n_cells * n_angles, which)
        for key in native.METRICS_DTYPE.names:       # what is asked for does not depend on what else is
            assert np.all(rec[key] == 0) or np.array_equal(rec[key].view(np.uint64), full[key].view(np.uint64)), (which, key)
    assert np.array_equal(ctx.compare_images(imgs, ref, ["ssim", "psnr"])["ssim"], full["ssim"])
    ctx.close()


def test_refusals_are_negative_with_a_message_and_write_nothing():
    ctx = conv_ctx(64, 16)
    L, h = ctx._L, ctx._h
    imgs, ref = image_set(2, 64, 16, seed=3)
    d_imgs, d_ref = torch.from_numpy(imgs).to(DEV), torch.from_numpy(ref).to(DEV)
    d_hist = torch.full((2, 256, 256), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    out = np.full(2 * 72, 0x5A, np.uint8)
    h_hist = np.full((2, 256, 256), 0x5A5A5A5A, np.uint32)
    o, i, r, dh = out.ctypes.data, d_imgs.data_ptr(), d_ref.data_ptr(), d_hist.data_ptr()

    def refused(rc, text):
        assert rc < 0, rc
        assert text in L.rr_last_error(h), L.rr_last_error(h)
    for win in (8, 2, 1, 17, -7, 0):
        refused(L.rr_compare_images_device(h, i, 2, r, ALL, win, o, dh, None), b"win_size")
    for which in (0, 8, 0xFFFFFFF8):
        refused(L.rr_compare_images_device(h, i, 2, r, which, 7, o, dh, None), b"which")
    for args in ((None, 2, r, ALL, 7, o, dh), (i, 2, None, ALL, 7, o, dh), (i, 2, r, ALL, 7, None, dh)):
        refused(L.rr_compare_images_device(h, *args, None), b"null buffer")
    for n in (0, 65536, -1):
        refused(L.rr_compare_images_device(h, i, n, r, ALL, 7, o, dh, None), b"n_images")
    refused(L.rr_compare_images_device(h, i, 2, r, native.METRIC_SSIM, 7, o, dh, None), b"RR_METRIC_INFO")
    refused(L.rr_compare_images(h, imgs.ctypes.data, 2, ref.ctypes.data, ALL, 8, o, h_hist.ctypes.data), b"rr_compare_images: win_size")
    refused(L.rr_compare_images(h, imgs.ctypes.data, 2, None, ALL, 7, o, h_hist.ctypes.data), b"null buffer")
    refused(L.rr_compare_images(h, imgs.ctypes.data, 2, ref.ctypes.data, 0, 7, o, h_hist.ctypes.data), b"which")
    refused(L.rr_simulate_param_sets_metrics(h, None, None, 1, 1, None, ref.ctypes.data, ALL, 8, o), b"win_size")
    refused(L.rr_simulate_param_sets_metrics(h, None, None, 1, 1, None, None, ALL, 7, o), b"null buffer")
    # an image smaller than the window: (1, 6, 400) with w = 7
    small = conv_ctx(6, 400)
    d6 = torch.zeros((6, 400), dtype=torch.uint8, device=DEV)
    assert small._L.rr_compare_images_device(small._h, d6.data_ptr(), 1, d6.data_ptr(), ALL, 7, o, None, None) == -3
    assert b"smaller than the window" in small._L.rr_last_error(small._h)
    torch.cuda.synchronize()
    assert np.all(out == 0x5A)
    ok = np.zeros(1, native.METRICS_DTYPE)
    assert small._L.rr_compare_images_device(small._h, d6.data_ptr(), 1, d6.data_ptr(), ALL, 5, ok.ctypes.data, None, None) == 0      # 5 fits
    assert ok["ssim"][0] == 1.0
    # a context without a config
    bare = native.Context(0)
    assert bare._L.rr_compare_images_device(bare._h, i, 2, r, ALL, 7, o, dh, None) == -2
    assert bare._L.rr_compare_images(bare._h, imgs.ctypes.data, 2, ref.ctypes.data, ALL, 7, o, None) == -2
    assert b"rr_set_config" in bare._L.rr_last_error(bare._h)
    torch.cuda.synchronize()
    assert np.all(out == 0x5A) and np.all(h_hist == 0x5A5A5A5A) and bool((d_hist == 0x5A5A5A5A).all())
    for c in (ctx, small, bare):
        c.close()


@pytest.fixture(scope="module")
def chain():
    """a small scene (config 2's, 2 passes, 200 cells of half a metre, noise off), 4 parameter sets, one reference image"""
    scene = scenes.config_scene(2)
    cfg = params.kaist_preset(n_reflections=2, n_samples=50, ambient_noise=0, n_cells=200, resolution=0.5)
    mats = materials_for(scene)
    ctx = native.Context(0)
    ctx.set_mesh(scene["verts"], scene["faces"], scene["face_object_id"])
    ctx.set_materials(mats, scene["object_materials"], 0)
    ctx.set_config(cfg, 400)
    ctx.set_beam_samples(golden_beams(50))
    pose = scenes.default_pose(scene["name"])
    m0 = np.array(mats_tuple(mats), np.float32)
    sets = []
    for k in range(4):
        m = m0.copy()
        m[1:, 1] *= 1.0 - 0.2 * k
        m[1:, 2] = 0.1 * k
        sets.append({"materials": m, "n_reflections": 1 + k % 2})
    real, _, _ = ctx.simulate(pose)
    yield ctx, pose, sets, len(mats), real
    ctx.close()


def test_param_sets_with_metrics_equal_compare_images_of_their_images(chain):
    ctx, pose, sets, n_mat, real = chain
    assert real.any()
    imgs, rec = ctx.simulate_param_sets(pose, sets, n_mat, ref_u8=real, metrics=ALL)
    assert imgs.shape == (4, 200, 400) and not np.array_equal(imgs[0], imgs[3])
    assert rec.tobytes() == ctx.compare_images(imgs, real).tobytes()
    plain, psnr = ctx.simulate_param_sets(pose, sets, n_mat, ref_u8=real)
    assert np.array_equal(plain, imgs) and np.array_equal(psnr.view(np.uint64), rec["psnr"].view(np.uint64))
    none, only = ctx.simulate_param_sets(pose, sets, n_mat, ref_u8=real, want_images=False, metrics=ALL)
    assert none is None and only.tobytes() == rec.tobytes()
    want = expected(imgs, real, 7, "chain")
    assert_records(rec, None, want, 200 * 400)
    assert np.all(np.isfinite(rec["ssim"])) and np.all(rec["mi"] > 0)
    _, ssim_only = ctx.simulate_param_sets(pose, sets, n_mat, ref_u8=real, want_images=False, metrics="ssim", win_size=11)
    assert np.all(ssim_only["psnr"] == 0) and np.all(ssim_only["hxy"] == 0)
    for k in range(4):
        assert abs(ssim_only["ssim"][k] - M.ssim(imgs[k], real, 11)) <= TOL


def test_python_facade_compare_images(chain):
    from radarays_ros_amd import radar
    ctx, pose, sets, n_mat, real = chain
    s = scenes.box12()
    r = radar.RadarHIP(s["verts"], s["faces"], s["face_object_id"])
    r.loadParams(params.kaist_materials(), s["object_materials"], 0)
    r.updateDynCfg(params.kaist_preset(n_reflections=1, ambient_noise=0, n_cells=200))
    imgs, ref = image_set(3, 200, 400, seed=12)
    rec = r.compareImages(list(imgs), ref)
    assert rec.tobytes() == r.context.compare_images(imgs, ref).tobytes()
    assert rec["ssim"][1] == 1.0 and r.compareImages(imgs[0], ref, "ssim")["ssim"][0] == rec["ssim"][0]


def test_cpp_mirror_compare_images(tmp_path):
    """RadarHIP::compareImages (include/radarays_ros_amd/RadarHIP.hpp) from a plain C++ program: the records of the ctypes path"""
    native.build()
    exe = str(tmp_path / "metrics_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "metrics_check.cpp"),
                    "-o", exe, "-L", os.path.join(ROOT, "radarays_ros_amd"), "-lradarays_mi355",
                    "-Wl,-rpath," + os.path.join(ROOT, "radarays_ros_amd")], check=True)
    n, n_cells, n_angles, win = 3, 120, 400, 9
    imgs, ref = image_set(n, n_cells, n_angles, seed=4)
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([n, n_cells, n_angles, ALL, win], np.int32).tobytes())
        f.write(ref.tobytes())
        f.write(imgs.tobytes())
    r = subprocess.run([exe, str(inp), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.frombuffer(open(out, "rb").read(), native.METRICS_DTYPE)
    ctx = conv_ctx(n_cells, n_angles)
    assert got.tobytes() == ctx.compare_images(imgs, ref, ALL, win).tobytes()
    assert_records(got, None, expected(imgs, ref, win, "cpp"), n_cells * n_angles)
    ctx.close()
