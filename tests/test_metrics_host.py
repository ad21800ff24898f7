"""Image metrics without a GPU: the numpy restatement (tests/metrics_ref.py) agrees with sklearn and with an integer form of
SSIM, metrics_from_joint_histogram regroups exact counts the way numpy bins the pixels, the feature's header text is as
stated (names, prototypes and layouts: tests/test_abi.py), the wrappers refuse bad arguments before any call into the library, and the
kernels of rr_metrics.hip use no scratch."""
import os
import re
import subprocess

import numpy as np
import pytest

import metrics_ref as M
from radarays_ros_amd import native, params, radar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radarays_ros_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "radarays_mi355.h")


def radar_like(shape, seed):
    """dark noise with sparse strong peaks, and a copy with 30 % of its pixels redrawn"""
    rs = np.random.RandomState(seed)
    ref = rs.randint(0, 30, shape).astype(np.uint8)
    peaks = rs.rand(*shape) < 0.02
    ref[peaks] = rs.randint(80, 256, int(peaks.sum()))
    img = ref.copy()
    hit = rs.rand(*shape) < 0.3
    img[hit] = rs.randint(0, 256, int(hit.sum()))
    return img, ref


def test_mutual_information_matches_sklearn():
    import sklearn.metrics as sk
    for shape, seed in (((64, 37), 1), ((100, 400), 2), ((7, 7), 3)):
        img, ref = radar_like(shape, seed)
        got = M.info(M.joint_histogram(img, ref))
        assert abs(got["mi"] - sk.mutual_info_score(img.ravel(), ref.ravel())) <= 1e-12
        assert abs(got["voi"] - (2 * got["hxy"] - got["hx"] - got["hy"])) == 0.0
        assert abs(got["nmi"] - (got["hx"] + got["hy"]) / got["hxy"]) == 0.0
    # hand-worked: two pixels in each of two bins, the images determine each other: hx = hy = hxy = mi = ln 2
    H = np.zeros((256, 256), np.uint32); H[0, 9] = 2; H[5, 0] = 2
    got = M.info(H)
    for k in ("hx", "hy", "hxy", "mi"):
        assert abs(got[k] - np.log(2.0)) <= 1e-15, k
    assert abs(got["nmi"] - 2.0) <= 1e-15 and abs(got["voi"]) <= 1e-15


def test_constant_images_have_zero_joint_entropy_and_nmi_one():
    H = M.joint_histogram(np.zeros((3424, 400), np.uint8), np.full((3424, 400), 255, np.uint8))
    assert H[0, 255] == 3424 * 400 and H.sum() == 3424 * 400
    got = M.info(H)
    assert got["hxy"] == 0.0 and got["hx"] == 0.0 and got["hy"] == 0.0 and got["nmi"] == 1.0 and got["mi"] == 0.0


@pytest.mark.parametrize("shape", [(7, 7), (64, 37), (100, 400), (3424, 400)])
def test_ssim_restatement_equals_the_integer_window_sum_form(shape):
    img, ref = radar_like(shape, shape[0])
    assert abs(M.ssim(img, ref) - M.ssim_integer(img, ref)) <= 1e-12
    assert M.ssim_integer(ref, ref) == 1.0
    if shape == (64, 37):
        for w in (3, 11, 15):
            assert abs(M.ssim(img, ref, w) - M.ssim_integer(img, ref, w)) <= 1e-12


def test_ssim_hand_worked_single_window():
    """one 3 x 3 window: x constant 10, y constant 20 -> no variance, S = (2 * 10 * 20 + C1) / (100 + 400 + C1)"""
    x, y = np.full((3, 3), 10, np.uint8), np.full((3, 3), 20, np.uint8)
    C1 = (0.01 * 255) ** 2
    assert abs(M.ssim_integer(x, y, 3) - (400 + C1) / (500 + C1)) <= 1e-15
    assert abs(M.ssim(x, y, 3) - (400 + C1) / (500 + C1)) <= 1e-12


@pytest.mark.parametrize("shape,seed", [((100, 400), 5), ((64, 37), 6)])
def test_histogram_regrouping_equals_numpy_binning_of_the_pixels(shape, seed):
    img, ref = radar_like(shape, seed)
    img[img > 200] = 200                       # the two images span different ranges
    ref[ref < 3] = 3
    H = M.joint_histogram(img, ref)
    got = native.metrics_from_joint_histogram(H, 100)
    B, _, _ = np.histogram2d(img.ravel(), ref.ravel(), bins=100)
    want = M.info(B)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-12, k
    import sklearn.metrics as sk
    full = native.metrics_from_joint_histogram(H)                 # one bin per grey level: nothing is regrouped
    assert abs(full["mi"] - sk.mutual_info_score(img.ravel(), ref.ravel())) <= 1e-12
    assert abs(full["nmi"] - (full["hx"] + full["hy"]) / full["hxy"]) <= 1e-15
    # one image constant: numpy widens its range by half a level on each side
    flat = np.full(shape, 17, np.uint8)
    got = native.metrics_from_joint_histogram(M.joint_histogram(flat, ref), 100)
    B, _, _ = np.histogram2d(flat.ravel(), ref.ravel(), bins=100)
    want = M.info(B)
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-12, k
    with pytest.raises(ValueError):
        native.metrics_from_joint_histogram(H[:255], 100)
    with pytest.raises(ValueError):
        native.metrics_from_joint_histogram(H, 0)


def test_metrics_entry_points_are_declared_and_exported(native_lib):
    """(names, argument types and struct layouts: tests/test_abi.py, for the whole header)"""
    header = open(HEADER).read()
    assert "#define RR_ABI_VERSION 7" in header
    for name, bit in (("RR_METRIC_PSNR", 1), ("RR_METRIC_SSIM", 2), ("RR_METRIC_INFO", 4)):
        assert re.search(r"#define %s %du" % (name, bit), header), name
    assert (native_lib.METRIC_PSNR, native_lib.METRIC_SSIM, native_lib.METRIC_INFO) == (1, 2, 4)
    assert "azimuth axis is not wrapped" in re.sub(r"[\s*]+", " ", header).lower()


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
    for which in (0, 8, -1, "sharpness", ["psnr", "x"], None, True):
        with pytest.raises(ValueError):
            o.compare_images(good, ref, which)
        with pytest.raises(ValueError):
            o.compare_images_device(1, 2, 1, which)
    for win in (2, 8, 1, 17, 7.0, "7"):
        with pytest.raises(ValueError):
            o.compare_images(good, ref, native.METRIC_SSIM, win)
    for bad in (np.zeros((2, 63, 16), np.uint8), np.zeros((2, 64, 16), np.float32)):
        with pytest.raises(ValueError):
            o.compare_images(bad, ref)
    with pytest.raises(ValueError):
        o.compare_images(good, np.zeros((2, 64, 16), np.uint8))
    with pytest.raises(ValueError):
        o.compare_images_device(None, 2, 1)
    for n in (0, 65536):
        with pytest.raises(ValueError):
            o.compare_images_device(1, n, 1)
    with pytest.raises(ValueError):
        o.simulate_param_sets(np.zeros(7), [{}], 1, ref_u8=None, metrics="ssim")
    assert native.metrics_mask(["psnr", "info"]) == 5 and native.metrics_mask("ssim") == 2 and native.metrics_mask(7) == 7


def test_radar_facade_has_the_metric_calls():
    assert callable(radar.RadarHIP.compareImages)
    hpp = open(os.path.join(ROOT, "include", "radarays_ros_amd", "RadarHIP.hpp")).read()
    assert "compareImages" in hpp and "rr_simulate_param_sets_metrics" in open(os.path.join(ROOT, "include", "radarays_ros_amd", "marshal.hpp")).read()


def test_metrics_kernels_use_no_scratch():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-metrics"], capture_output=True, text=True, timeout=600)
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
    for k in ("k_joint_hist", "k_ssim", "k_metrics_finish"):
        assert k in names, (k, sorted(rows))
    assert len(rows) == 4                                                  # two histogram shapes
    for name, u in rows.items():
        assert u["scratch"] == 0, (name, u)
        if "k_joint_histILb1" in name:
            assert u["lds"] == 128 * 1024, (name, u)                       # 32,768 words of two 16-bit counts
        elif "k_joint_hist" in name:
            assert u["lds"] == 0, (name, u)
        else:
            assert u["lds"] <= 2048, (name, u)                             # static; k_ssim's tiles are dynamic (<= 54 KB)


def test_metrics_source_is_in_the_library_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rr_metrics.hip" in src
    assert re.search(r"^resource-usage-metrics:", mk, re.M)
