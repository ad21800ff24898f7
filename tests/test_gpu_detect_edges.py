"""The kernels of rr_detect.hip at their tiling edges against the numpy restatement (tests/detect_ref.py).  The cases and the proof
that each one reaches its edge are in tests/test_detect_edges_host.py; its docstring lists the boundaries covered and those that are
not.  Every detector case goes through the device form (rr_detect_device, canaries behind both outputs and one spare row) and the host
form (rr_detect) on a context with a config and no mesh: offsets, column, bin and intensity exact, x and y within the 1e-6 r + 1e-6 of
tests/test_gpu_detect.py.  Image bases 1, 4 and 8 bytes past an aligned allocation go through the device form on a TW = 16 and a TW = 4
shape whose azimuth count would allow row loads: at 4 bytes the 16-wide tile must fall to byte loads while the 4-wide one keeps words.
The Cartesian cases are held to the two rules of test_cartesian_matches_the_restatement (nearest: at most max(1, 1e-3 * size) pixels
differ and each reads a neighbouring cell; bilinear: off by at most 1 on at most 1e-3 of the pixels), with canaries on both sides of
the device output."""
import numpy as np
import pytest

import test_detect_edges_host as H
from radarays_ros_amd import native
from test_gpu_detect import assert_frame, config, geometry

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
CANARY = 0xA5


def ctx_for(c):
    """a context with the case's config and no mesh"""
    ctx = native.Context(0)
    ctx.set_config(config(c.n_cells, c.scroll), c.n_angles, **H.config_kw(c))
    assert geometry(ctx) == H.geometry(c)
    return ctx


def device_images(imgs, offset):
    """the images `offset` bytes past an aligned device allocation -> (the allocation, the images' address)"""
    buf = torch.zeros(imgs.size + offset + 16, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    buf[offset:offset + imgs.size] = torch.from_numpy(imgs.ravel()).to(DEV)
    return buf, buf.data_ptr() + offset


def detect_device(ctx, imgs, det, want, offset=0):
    """rr_detect_device into canary-filled buffers one row longer than needed -> (points per frame, offsets); nothing but the
    detections and the offsets may have been written"""
    n, _, n_angles = imgs.shape
    mp = max(1, max(int(offs[-1]) for _, offs in want))
    buf, ptr = device_images(imgs, offset)
    pts = torch.full(((n + 1) * mp * 24,), CANARY, dtype=torch.uint8, device=DEV)
    offs = torch.full(((n + 1) * (n_angles + 1) * 4,), CANARY, dtype=torch.uint8, device=DEV)
    ctx.detect_device(ptr, n, det, pts.data_ptr(), mp, offs.data_ptr())
    ctx.synchronize()
    h_offs = offs.cpu().numpy().view(np.uint32).reshape(n + 1, n_angles + 1)
    h_pts = pts.cpu().numpy().reshape(n + 1, mp * 24)
    assert np.all(h_offs[n] == 0xA5A5A5A5) and np.all(h_pts[n] == CANARY)
    out = []
    for f in range(n):
        total = int(h_offs[f, -1])
        assert total == int(want[f][1][-1]) <= mp, (f, total)
        assert np.all(h_pts[f, total * 24:] == CANARY), f
        out.append(h_pts[f, :total * 24].view(native.POINT_DTYPE))
    return out, h_offs[:n]


def check(got, want):
    pts, offs = got
    assert len(pts) == len(want)
    for f, (want_pts, want_offs) in enumerate(want):
        assert_frame(pts[f], offs[f], want_pts, want_offs)


@pytest.mark.parametrize("name", H.DET_IDS)
def test_detector_case_matches_the_restatement(name):
    c = H.DET_CASES[H.DET_IDS.index(name)]
    ctx = ctx_for(c)
    imgs, want = H.frames(c), H.want(c)
    check(detect_device(ctx, imgs, c.det, want), want)
    check(ctx.detect(imgs, c.det), want)
    total = sum(int(offs[-1]) for _, offs in want)
    assert (total == 0) == (c.expect == "none")


@pytest.mark.parametrize("offset", H.UNALIGNED_OFFSETS)
@pytest.mark.parametrize("name", [c.name for c in H.UNALIGNED])
def test_images_at_unaligned_bases(name, offset):
    c = next(u for u in H.UNALIGNED if u.name == name)
    ctx = ctx_for(c)
    imgs, want = H.frames(c), H.want(c)
    check(detect_device(ctx, imgs, c.det, want, offset), want)
    assert sum(int(offs[-1]) for _, offs in want) > 0


def cartesian_device(ctx, imgs, c):
    """rr_polar_to_cartesian_device into the middle of a canary-filled buffer, out_offset bytes past an aligned address"""
    n, total = len(imgs), len(imgs) * c.width * c.width
    buf, ptr = device_images(imgs, 0)
    front = 16 + c.out_offset
    out = torch.full((front + total + 64,), CANARY, dtype=torch.uint8, device=DEV)
    assert out.data_ptr() % 16 == 0
    ctx.polar_to_cartesian_device(ptr, n, c.width, H.pixel_size(c), out.data_ptr() + front, c.bilinear)
    ctx.synchronize()
    h = out.cpu().numpy()
    assert np.all(h[:front] == CANARY) and np.all(h[front + total:] == CANARY)
    return h[front:front + total].reshape(n, c.width, c.width)


def assert_cartesian(got, imgs, c):
    """the two rules of tests/test_gpu_detect.py::test_cartesian_matches_the_restatement, at any azimuth count"""
    A, N = c.n_angles, c.n_cells
    assert got.shape == (len(imgs), c.width, c.width)
    for f in range(len(imgs)):
        if c.bilinear:
            d = np.abs(got[f].astype(int) - H.cart_want(c.name, f))
            print("%s frame %d: max difference %d on %.2e of the pixels" % (c.name, f, d.max(), np.mean(d > 0)))
            assert d.max() <= 1 and np.mean(d > 0) <= 1e-3, (f, d.max(), np.mean(d > 0))
            continue
        want, b, a, outside = H.cart_want(c.name, f)
        bad = np.nonzero(got[f] != want)
        print("%s frame %d: %d of %d pixels differ" % (c.name, f, len(bad[0]), want.size))
        assert len(bad[0]) <= max(1, 1e-3 * want.size), (f, len(bad[0]))
        for i, j in zip(*bad):                           # a flipped rounding reads a neighbouring cell
            if outside[i, j]:
                ok = {0} | {int(imgs[f][N - 1, (a[i, j] + da + c.scroll) % A]) for da in (-1, 0, 1)}
            else:
                ok = {int(imgs[f][min(max(b[i, j] + db, 0), N - 1), (a[i, j] + da + c.scroll) % A])
                      for db in (-1, 0, 1) for da in (-1, 0, 1)}
            assert int(got[f][i, j]) in ok, (f, i, j)


@pytest.mark.parametrize("name", H.CART_IDS)
def test_cartesian_case_matches_the_restatement(name):
    c = H.CART_CASES[H.CART_IDS.index(name)]
    ctx = ctx_for(c)
    imgs = H.cart_frames(c)
    assert_cartesian(cartesian_device(ctx, imgs, c), imgs, c)
    if not c.out_offset:
        assert_cartesian(ctx.polar_to_cartesian(imgs, c.width, H.pixel_size(c), c.bilinear), imgs, c)
