"""Azimuth registration without a GPU: the numpy restatement (tests/align_ref.py) agrees with the literal np.roll definition
and with hand-worked cases, the feature's header text (names, prototypes and layouts: tests/test_abi.py), the wrappers
refuse bad arguments before any call into the library, and the kernels of rr_align.hip use no scratch and the LDS their
header states."""
import os
import re
import subprocess

import numpy as np
import pytest

import align_ref as A
import metrics_ref as M
from radarays_ros_amd import native, params, radar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radarays_ros_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "radarays_mi355.h")


def pair(shape, seed):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, shape).astype(np.uint8), rs.randint(0, 256, shape).astype(np.uint8)


@pytest.mark.parametrize("shape", [(7, 5), (64, 37), (100, 400)])
def test_restatement_equals_the_roll_definition_for_every_shift(shape):
    x, r = pair(shape, shape[0])
    assert np.array_equal(A.xcorr(x, r), A.xcorr_roll(x, r))
    cb, ce = shape[0] // 3, shape[0] - 1
    assert np.array_equal(A.xcorr(x, r, cb, ce), A.xcorr_roll(x, r, cb, ce))
    # a rolled copy is found at n_angles - k, with no error left
    k = 2
    got = A.align(np.roll(r, k, axis=1), r)
    assert got["shift"] == shape[1] - k and got["sse"] == 0 and got["psnr"] == np.inf and got["ncc"] == 1.0 and got["n_best"] == 1


@pytest.mark.parametrize("a0,a1", [(5, 30), (30, 5)])
def test_hand_worked_single_pixels(a0, a1):
    """x has one pixel of value 3 at (c0, a0), r one of value 5 at (c0, a1): 15 at s = (a1 - a0) mod n_angles, 0 elsewhere"""
    n_cells, n_angles, c0 = 64, 37, 9
    x, r = np.zeros((n_cells, n_angles), np.uint8), np.zeros((n_cells, n_angles), np.uint8)
    x[c0, a0], r[c0, a1] = 3, 5
    want = np.zeros(n_angles, np.int64)
    want[(a1 - a0) % n_angles] = 15
    assert np.array_equal(A.xcorr(x, r), want) and np.array_equal(A.xcorr_roll(x, r), want)
    got = A.align(x, r)
    assert got["shift"] == (a1 - a0) % n_angles and got["n_best"] == 1 and got["xcorr"] == 15 and got["sse"] == 9 + 25 - 30
    assert (got["sum_x"], got["sum_xx"], got["sum_r"], got["sum_rr"]) == (3, 9, 5, 25)
    assert np.all(A.xcorr(x, r, c0 + 1, n_cells) == 0)                 # the pixel's row left out of the window


def test_sse_at_shift_zero_is_the_psnr_restatements_sse():
    for shape in ((64, 37), (100, 400)):
        x, r = pair(shape, 11)
        c = A.xcorr(x, r)
        xi, ri = x.astype(np.int64), r.astype(np.int64)
        sse, psnr = M.psnr(x, r)
        assert int((xi * xi).sum() + (ri * ri).sum() - 2 * c[0]) == sse
        assert A.psnr_of(sse, x.size) == psnr


def test_align_entry_points_are_declared_and_exported(native_lib):
    """(names, argument types and struct layouts: tests/test_abi.py, for the whole header)"""
    header = open(HEADER).read()
    assert "#define RR_ABI_VERSION 7" in header
    assert "typedef struct rr_align_record" in header


def _unopened(n_cells=64, n_angles=16):
    o = native.Context.__new__(native.Context)
    o._h = None
    o._L = None
    o.cfg = params.RadarModelConfig(n_cells=n_cells)
    o.n_angles = n_angles
    return o


def test_wrappers_refuse_bad_arguments_before_the_library():
    o = _unopened()
    good, ref = np.zeros((2, 64, 16), np.uint8), np.zeros((64, 16), np.uint8)
    for cb, ce in ((-1, 64), (0, 65), (5, 5), (6, 5), (64, None), (0, 0), (0.0, 64), (0, "64"), (True, 64)):
        with pytest.raises(ValueError):
            o.align_images(good, ref, cb, ce)
        with pytest.raises(ValueError):
            o.align_images_device(1, 2, 1, cb, ce)
        with pytest.raises(ValueError):
            o.simulate_batch_align(np.zeros((1, 7)), ref, cb, ce)
    for bad in (np.zeros((2, 63, 16), np.uint8), np.zeros((2, 64, 16), np.float32), np.zeros((2, 64, 17), np.uint8)):
        with pytest.raises(ValueError):
            o.align_images(bad, ref)
    with pytest.raises(ValueError):
        o.align_images(good, np.zeros((2, 64, 16), np.uint8))
    with pytest.raises(ValueError):
        o.align_images(good, np.zeros((64, 16), np.int8))
    with pytest.raises(ValueError):
        o.align_images_device(None, 2, 1)
    with pytest.raises(ValueError):
        o.align_images_device(1, 2, None)
    for n in (0, 65536, 2.0):
        with pytest.raises(ValueError):
            o.align_images_device(1, n, 1)
    for poses in (np.zeros((0, 7)), np.zeros((65, 7)), np.zeros((2, 6)), [["a"] * 7]):
        with pytest.raises(ValueError):
            o.simulate_batch_align(poses, ref)
    with pytest.raises(ValueError):
        o.simulate_batch_align(np.zeros((1, 7)), good)
    # a window of more than 2^23 pixels
    big = _unopened(n_cells=8192, n_angles=1025)
    with pytest.raises(ValueError):
        big.align_images_device(1, 1, 1)
    assert big._cell_window(8, 8192) == (8, 8192)             # 8184 x 1025 = 8,388,600 <= 2^23
    with pytest.raises(ValueError):
        big._cell_window(7, 8192)


def test_radar_facade_has_the_align_call():
    assert callable(radar.RadarHIP.alignImages)
    hpp = open(os.path.join(ROOT, "include", "radarays_ros_amd", "RadarHIP.hpp")).read()
    assert "alignImages" in hpp and "rr_align_images" in open(os.path.join(ROOT, "include", "radarays_ros_amd", "marshal.hpp")).read()


def test_align_kernels_use_no_scratch_and_the_lds_their_header_states():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-align"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    rows, cur = {}, None
    for line in (r.stdout + r.stderr).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        for key, name in ((r"ScratchSize \[bytes/lane\]", "scratch"), (r"LDS Size \[bytes/block\]", "lds")):
            m = re.search(r"remark:\s+" + key + r": (\d+)", line)
            if m and cur is not None:
                cur[name] = int(m.group(1))
    head = open(os.path.join(CSRC, "rr_align.hip")).read().split("#include")[0]
    stated = {"k_align_gram": 45692, "k_align_finish": 3080, "k_align_sums": 0}
    assert "k_align_gram 45,692 B" in head and "k_align_finish 3,080 B" in head and "k_align_sums none" in head
    assert len(rows) == 3, sorted(rows)
    for k, lds in stated.items():
        hit = [u for name, u in rows.items() if k in name]
        assert len(hit) == 1, (k, sorted(rows))
        assert hit[0]["scratch"] == 0 and hit[0]["lds"] <= lds, (k, hit[0])


def test_align_source_is_in_the_library_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rr_align.hip" in src
    assert re.search(r"^resource-usage-align:", mk, re.M)
    assert "k_align" not in open(os.path.join(CSRC, "rr_metrics.hip")).read()
