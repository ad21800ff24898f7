"""Point clouds and Cartesian images without a GPU: the numpy restatement (tests/detect_ref.py) gives hand-worked answers on tiny
columns (names, prototypes and struct layouts: tests/test_abi.py), the Python wrappers refuse bad shapes and configs before any call into the library, and the kernels of rr_detect.hip use no scratch."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import detect_ref as R
from radarays_ros_amd import native, params, radar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radarays_ros_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "radarays_mi355.h")


def test_detect_entry_points_are_declared_and_exported(native_lib):
    """(names, argument types and struct layouts: tests/test_abi.py, for the whole header)"""
    header = open(HEADER).read()
    assert "#define RR_ABI_VERSION 7" in header
    assert native_lib.lib().rr_abi_version() == 7


def test_default_detect_config_matches_the_python_defaults(native_lib):
    c = native_lib.RRDetectConfig()
    native_lib.lib().rr_default_detect_config(ctypes.byref(c))
    assert {k: getattr(c, k) for k in native_lib.DETECT_DEFAULTS} == native_lib.DETECT_DEFAULTS


# ---- the restatement on hand-worked columns ---------------------------------------------------------------------------
def col(values):
    return np.asarray(values, np.uint8)[:, None]


def bins(mask):
    return list(np.nonzero(mask[:, 0])[0])


def test_cfar_lone_peak_with_one_training_cell():
    assert bins(R.cfar_mask(col([0, 0, 9, 0, 0]), guard=0, train=1, min_intensity=1, scale=1.0)) == [2]
    # an empty cell never beats an empty window (0 > 0 is false), and a cell beside the peak is below it
    assert bins(R.cfar_mask(col([0, 0, 9, 0, 0]), guard=0, train=1, min_intensity=0, scale=1.0)) == [2]
    # a wide target: with G = 1 the middle bin's window is bins 0 and 4 (empty), bin 1's is bin 3 alone (9 > 9 is false)
    assert bins(R.cfar_mask(col([0, 9, 9, 9, 0]), guard=1, train=1, min_intensity=1, scale=1.0)) == [2]
    # with G = 0 the middle bin's neighbours mask it (18 > 18 is false) and the edges stand out against one empty cell
    assert bins(R.cfar_mask(col([0, 9, 9, 9, 0]), guard=0, train=1, min_intensity=1, scale=1.0)) == [1, 3]


def test_cfar_windows_are_clipped_at_both_ends():
    # bin 0: no left cells, right = {1, 2}: n = 2, S = 2, 5 * 2 = 10 > 2; bin 2: left = {0, 1}: 1 * 2 = 2 > 6 is false
    assert bins(R.cfar_mask(col([5, 1, 1]), guard=0, train=2, scale=1.0, min_intensity=0)) == [0]
    assert bins(R.cfar_mask(col([1, 1, 5]), guard=0, train=2, scale=1.0, min_intensity=0)) == [2]
    # the comparison is strict and in f32: 2 * 4 = 8 against scale * S = 2 * 4
    assert bins(R.cfar_mask(col([2, 4, 2]), guard=0, train=1, scale=2.0, min_intensity=0)) == []
    assert bins(R.cfar_mask(col([2, 4, 2]), guard=0, train=1, scale=1.99, min_intensity=0)) == [1]


def test_cfar_without_training_cells_detects_nothing():
    assert bins(R.cfar_mask(col([200]), guard=0, train=4, scale=0.0, min_intensity=0)) == []
    assert bins(R.cfar_mask(col([200, 0, 0]), guard=5, train=1, scale=0.0, min_intensity=0)) == []
    # scale 0: every cell with training cells and a nonzero value
    assert bins(R.cfar_mask(col([200, 0, 3]), guard=0, train=1, scale=0.0, min_intensity=0)) == [0, 2]


def test_kstrongest_breaks_ties_by_bin():
    z = col([3, 7, 7, 2, 7])
    assert bins(R.kstrongest_mask(z, 2)) == [1, 2]
    assert bins(R.kstrongest_mask(z, 3)) == [1, 2, 4]
    assert bins(R.kstrongest_mask(z, 4)) == [0, 1, 2, 4]
    assert bins(R.kstrongest_mask(z, 5)) == [0, 1, 2, 3, 4]


def test_min_bin_and_min_intensity():
    z = col([9, 9, 1, 5, 4])
    assert bins(R.kstrongest_mask(z, 3, min_intensity=4, min_bin=1)) == [1, 3, 4]
    assert bins(R.kstrongest_mask(z, 2, min_intensity=4, min_bin=1)) == [1, 3]
    assert bins(R.kstrongest_mask(z, 9, min_intensity=6)) == [0, 1]
    assert bins(R.cfar_mask(col([9, 0, 0, 0]), guard=0, train=1, scale=1.0, min_bin=0)) == [0]
    assert bins(R.cfar_mask(col([9, 0, 0, 0]), guard=0, train=1, scale=1.0, min_bin=1)) == []
    # cells below min_bin still train: the 9 at bin 0 hides the 4 at bin 1
    assert bins(R.cfar_mask(col([9, 4, 0, 0]), guard=0, train=1, scale=1.0, min_bin=1, min_intensity=1)) == []


def test_frame_points_order_offsets_and_geometry():
    img = np.zeros((6, 4), np.uint8)
    img[5, 3] = 50; img[1, 0] = 60; img[2, 0] = 70
    pts, offs = R.detect_frame(img, method=1, k=1, min_intensity=1, scroll=1, theta_min=0.0, theta_inc=-np.pi / 2, resolution=2.0)
    assert list(pts["column"]) == [0, 3] and list(pts["bin"]) == [2, 5]
    assert list(offs) == [0, 1, 1, 1, 2]
    # column 0 holds azimuth (0 - 1) mod 4 = 3 (yaw -3 pi / 2: +y); bin 2 lies at 5 m
    assert np.allclose([pts["x"][0], pts["y"][0]], [0.0, 5.0], atol=1e-5)
    # column 3 holds azimuth 2 (yaw -pi: -x); bin 5 at 11 m
    assert np.allclose([pts["x"][1], pts["y"][1]], [-11.0, 0.0], atol=1e-5)
    assert list(pts["intensity"]) == [70.0, 50.0] and np.all(pts["z"] == 0)


def test_cartesian_restatement_on_a_ring():
    """every bin of the polar image set to its bin number: a Cartesian pixel at range rho reads bin ~ rho / res - 0.5"""
    img = np.tile(np.arange(50, dtype=np.uint8)[:, None], (1, 400))
    out = R.cartesian(img, 21, 1.0, bilinear=False, resolution=1.0)
    assert out[10, 10] == 0                                         # the centre: v = -0.5 clamps to bin 0
    assert out[10, 0] == 10 and out[0, 10] == 10                    # 10 m left / ahead: v = 9.5 rounds half-even to bin 10
    assert out[10, 13] == 2                                         # 3 m right: v = 2.5 -> 2
    lin = R.cartesian(img, 21, 1.0, bilinear=True, resolution=1.0)
    assert lin[10, 13] == 2 and lin[10, 0] == 10                    # 2.5 -> rint(2.5) = 2; 9.5 -> 10
    far = R.cartesian(img, 201, 1.0, bilinear=True, resolution=1.0)
    assert far[0, 0] == 0 and far[100, 100 - 49] == 48              # past the last bin: 0; 49 m: v = 48.5, lerp 48.5 -> 48
    assert far[100, 100 - 60] == 0


# ---- wrappers refuse before the library -------------------------------------------------------------------------------
def _unopened(n_cells=64, n_angles=16):
    o = native.Context.__new__(native.Context)
    o._h = None
    o._L = None
    o.cfg = params.RadarModelConfig(n_cells=n_cells)
    o.n_angles = n_angles
    return o


def test_wrappers_refuse_bad_images_before_the_library():
    o = _unopened()
    good = np.zeros((2, 64, 16), np.uint8)
    for bad in (np.zeros((2, 64, 16), np.float32), np.zeros((2, 63, 16), np.uint8), np.zeros((2, 64, 17), np.uint8),
                np.zeros((64,), np.uint8), np.zeros((1, 2, 64, 16), np.uint8), np.zeros((0, 64, 16), np.uint8)):
        with pytest.raises(ValueError):
            o.detect(bad)
        with pytest.raises(ValueError):
            o.polar_to_cartesian(bad, 32, 0.5)
    with pytest.raises(native.RRError, match="rr_set_config"):
        u = _unopened(); u.cfg = None; u.detect(good)
    assert good.sum() == 0


@pytest.mark.parametrize("bad", [dict(method=2), dict(method="median"), dict(guard_cells=-1), dict(guard_cells=1025),
                                 dict(train_cells=0), dict(train_cells=1025), dict(k=0), dict(k=65), dict(min_intensity=-1),
                                 dict(min_intensity=256), dict(min_bin=-1), dict(min_bin=64), dict(cfar_scale=-0.5),
                                 dict(cfar_scale=float("nan")), dict(cfar_scale=float("inf")), dict(cfar_scale=1e39),
                                 dict(k=2.5), dict(bogus=1)])
def test_wrappers_refuse_bad_detect_configs_before_the_library(bad):
    o = _unopened()
    img = np.zeros((1, 64, 16), np.uint8)
    with pytest.raises(ValueError):
        o.detect(img, **bad)
    with pytest.raises(ValueError):
        o.detect_device(1, 1, d_offsets_ptr=1, **bad)


def test_wrappers_refuse_bad_cartesian_configs_and_counts_before_the_library():
    o = _unopened()
    img = np.zeros((1, 64, 16), np.uint8)
    for w, ps in ((0, 1.0), (8193, 1.0), (2.5, 1.0), (16, 0.0), (16, -1.0), (16, float("nan")), (16, float("inf")), (16, 1e-50)):
        with pytest.raises(ValueError):
            o.polar_to_cartesian(img, w, ps)
        with pytest.raises(ValueError):
            o.polar_to_cartesian_device(1, 1, w, ps, 1)
    for n in (0, 65536, -1):
        with pytest.raises(ValueError):
            o.detect_device(1, n, d_offsets_ptr=1)
        with pytest.raises(ValueError):
            o.polar_to_cartesian_device(1, n, 16, 1.0, 1)
    with pytest.raises(ValueError):
        o.detect_device(1, 1, d_offsets_ptr=1, max_points=-1)
    with pytest.raises(ValueError):
        o.detect_device(1, 1, d_offsets_ptr=None)
    with pytest.raises(ValueError):
        o.detect_device(1, 1, d_offsets_ptr=1, max_points=4, d_points_ptr=None)
    with pytest.raises(ValueError):
        o.detect(img, max_points=-1)


def test_radar_facade_has_the_conversion_calls():
    for n in ("toPointCloud", "toCartesian", "simulatePointClouds"):
        assert callable(getattr(radar.RadarHIP, n)), n


# ---- kernels ----------------------------------------------------------------------------------------------------------
def test_detect_kernels_use_no_scratch():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-detect"], capture_output=True, text=True, timeout=600)
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
    names = " ".join(rows)
    for k in ("k_detect", "k_detect_scan", "k_cartesian"):
        assert k in names, (k, sorted(rows))
    assert len([n for n in rows if "k_detectIL" in n]) == 8              # 2 tile widths x 2 methods x count / emit
    for name, u in rows.items():
        assert u["scratch"] == 0 and u["lds"] <= 1024, (name, u)         # static LDS; the tile is dynamic (<= 64 KB)


def test_detect_source_is_in_the_library_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rr_detect.hip" in src
    assert re.search(r"^resource-usage-detect:", mk, re.M)
