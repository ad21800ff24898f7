"""Windowed CFAR without a GPU: the entry points exist under ABI 7, every refusal of the header is made before anything is written, the
reported tile respects its limits, the numpy restatement (tests/window_ref.py) agrees with its own literal form, with rr_detect's CA-CFAR
where the two coincide and with hand-worked ranks, the wall scene of DESIGN.md section 33, the threshold table the OS kernel counts
against, and the kernels of rr_window.hip use no scratch."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import detect_ref
import window_ref as W
from radarays_ros_amd import native, params, radar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radarays_ros_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "radarays_mi355.h")


def synthetic(n_frames, n_cells, n_angles, seed):
    """test_gpu_detect.synthetic's frames: low noise with sparse strong peaks (peaks at bin 0 and n_cells - 1 too)"""
    rs = np.random.RandomState(seed)
    imgs = rs.randint(0, 30, (n_frames, n_cells, n_angles)).astype(np.uint8)
    peaks = rs.rand(n_frames, n_cells, n_angles) < 0.02
    imgs[peaks] = rs.randint(80, 256, int(peaks.sum()))
    imgs[:, 0, ::3] = 240
    imgs[:, n_cells - 1, 1::3] = 250
    return imgs


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_window_entry_points_are_exported_under_abi_7(native_lib):
    assert "#define RR_ABI_VERSION 7" in open(HEADER).read()
    L = native_lib.lib()
    assert L.rr_abi_version() == 7
    for n in ("rr_default_window_detect_config", "rr_detect_window_device", "rr_detect_window", "rr_detect_window_tile_sizes"):
        assert hasattr(L, n) and n in native_lib.PROTOTYPES, n
    assert C.sizeof(native_lib.RRWindowDetectConfig) == 48


def test_default_window_config_matches_the_python_defaults(native_lib):
    c = native_lib.RRWindowDetectConfig()
    native_lib.lib().rr_default_window_detect_config(C.byref(c))
    assert {k: getattr(c, k) for k in native_lib.WINDOW_DEFAULTS} == native_lib.WINDOW_DEFAULTS
    assert native_lib.WINDOW_DEFAULTS == W.DEFAULTS and not any(c.reserved_)


# ---- refusals -------------------------------------------------------------------------------------------------------------
def raw_cfg(L, **kw):
    c = native.RRWindowDetectConfig()
    L.rr_default_window_detect_config(C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


# every -3 of the header's config for images of 64 bins by 64 columns (tests/test_gpu_window.py sends them to the device and host forms)
BAD = [dict(method=4), dict(method=-1), dict(guard_range=-1), dict(guard_range=1025), dict(train_range=-1), dict(train_range=1025),
       dict(guard_azimuth=-1), dict(guard_azimuth=33), dict(train_azimuth=-1), dict(train_azimuth=33), dict(rank_permille=0),
       dict(rank_permille=1001), dict(min_intensity=-1), dict(min_intensity=256), dict(min_bin=-1), dict(min_bin=64), dict(scale=-1.0),
       dict(scale=float("nan")), dict(scale=float("inf")),
       dict(train_range=0, train_azimuth=0),                                    # no training cells
       dict(guard_azimuth=16, train_azimuth=16),                                # 65 columns on a circle of 64
       dict(guard_range=1024, train_range=1024, guard_azimuth=4, train_azimuth=4),   # 4097 x 17 = 69,649 cells (x 15 = 61,455 is allowed)
       dict(method=1, train_range=0), dict(method=2, train_range=0)]


def test_tile_sizes_refuse_what_the_detector_refuses(native_lib):
    L = native_lib.lib()
    out = (C.c_int * 4)(-7, -7, -7, -7)
    for kw in BAD:
        assert L.rr_detect_window_tile_sizes(C.byref(raw_cfg(L, **kw)), 64, 64, out) == -3, kw
    assert L.rr_detect_window_tile_sizes(None, 64, 16, out) == -3
    assert L.rr_detect_window_tile_sizes(C.byref(raw_cfg(L)), 0, 16, out) == -3
    assert L.rr_detect_window_tile_sizes(C.byref(raw_cfg(L)), 64, 16, None) == -3
    assert list(out) == [-7] * 4
    # 4097 rows by 15 columns: 61,455 cells, inside the bound
    assert L.rr_detect_window_tile_sizes(C.byref(raw_cfg(L, guard_range=1024, train_range=1024, guard_azimuth=3, train_azimuth=4)), 64, 16, out) == 0


@pytest.mark.parametrize("bad", BAD + [dict(method="median"), dict(scale=1e39), dict(rank_permille=2.5), dict(bogus=1)])
def test_wrappers_refuse_bad_window_configs_before_the_library(bad):
    with pytest.raises(ValueError):
        native.window_detect_config(n_cells=64, n_angles=64, **bad)
    o = native.Context.__new__(native.Context)
    o._h = o._L = None
    o.cfg, o.n_angles = params.RadarModelConfig(n_cells=64), 64
    with pytest.raises(ValueError):
        o.detect_window(np.zeros((1, 64, 64), np.uint8), **bad)
    with pytest.raises(ValueError):
        o.detect_window_device(1, 1, d_offsets_ptr=1, **bad)


def test_tile_sizes_are_consistent_with_the_limits(native_lib):
    """The strip narrows as n_cells grows (16 columns up to 1024 bins, 8 up to 2048, 4 beyond), so the workgroup count grows with it.  The
    halo is the window's.  The step's staged bytes -- rows of 16-byte words where n_angles % 16 == 0, the first of them up to 15 columns left
    of the halo, plus the two uint16 row-sum planes of CA / GO / SO -- fit the 160 KB of a CU, twice wherever the smallest tile does.  A
    chunk of the step, its rows over the 256 / columns threads of a column, is at most 16 bins: its detections fit one word."""
    windows = [dict(), dict(guard_range=0, train_range=1, guard_azimuth=0, train_azimuth=1), dict(guard_range=1024, train_range=1024, guard_azimuth=0, train_azimuth=1),
               dict(guard_range=0, train_range=253, guard_azimuth=32, train_azimuth=32), dict(guard_range=400, train_range=500, guard_azimuth=8, train_azimuth=8),
               dict(guard_range=0, train_range=0, guard_azimuth=0, train_azimuth=1), dict(guard_range=3, train_range=1024, guard_azimuth=0, train_azimuth=0)]

    def staged(rows, cols, Hr, Hc, method, n_angles):
        if n_angles % 16:
            w = cols + 2 * Hc
        else:
            w = 16 + 2 * (-(-Hc // 16) * 16) if cols == 16 else -(-(15 + Hc + cols + Hc) // 16) * 16
        return (rows + 2 * Hr) * w + (0 if method == 3 else (rows + 2 * Hr) * cols * 4)

    for w in windows:
        for method in (0, 3):
            for n_angles in (400, 401):
                for n_cells, top in ((300, 16), (1024, 16), (1025, 8), (2048, 8), (2049, 4), (4000, 4)):
                    cfg = dict(w, method=method)
                    rows, cols, hr, hc = native_lib.detect_window_tile_sizes(cfg, n_cells, n_angles)
                    c = W.config(**cfg)
                    Hr, Hc = c["guard_range"] + c["train_range"], c["guard_azimuth"] + c["train_azimuth"]
                    assert rows in (32, 64, 128, 256, 512, 1024) and cols in (1, 2, 4, 8, 16) and cols <= top, (cfg, rows, cols)
                    assert (hr, hc) == (Hr, Hc)
                    lds = staged(rows, cols, Hr, Hc, method, n_angles)
                    assert lds + 2048 <= 160 * 1024, (cfg, lds)
                    if staged(32, 1, Hr, Hc, method, n_angles) + 2048 <= 80 * 1024:
                        assert lds + 2048 <= 80 * 1024, (cfg, lds)
                    assert -(-rows // (256 // cols)) <= 16
    # the default window takes the widest strip and the tallest step of its class; the grid grows with n_cells
    sizes = {n: native_lib.detect_window_tile_sizes(dict(), n, 400)[:2] for n in (512, 1024, 2048, 3424)}
    assert sizes == {512: (256, 16), 1024: (256, 16), 2048: (512, 8), 3424: (1024, 4)}
    groups = [-(-400 // sizes[n][1]) for n in (1024, 2048, 3424)]
    assert groups == [25, 50, 100]


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [dict(guard_range=1, train_range=2, guard_azimuth=1, train_azimuth=1, rank_permille=600, scale=1.5, min_bin=1),
                                    dict(guard_range=0, train_range=1, guard_azimuth=0, train_azimuth=1, rank_permille=500, scale=1.0, min_intensity=0),
                                    dict(guard_range=0, train_range=9, guard_azimuth=2, train_azimuth=0, rank_permille=1000, scale=2.0),
                                    dict(guard_range=2, train_range=0, guard_azimuth=0, train_azimuth=2, rank_permille=1, scale=0.0)])
def test_whole_image_restatement_equals_the_literal_definition(window):
    """masks (shifted copies, summed or sorted) against cell (loops and sorted()) at every cell: clipped rows at both ends (the image is
    shorter than some windows), wrapped columns, a window that is the whole circle"""
    rs = np.random.RandomState(11)
    img = rs.randint(0, 40, (14, 5)).astype(np.uint8)
    img[rs.rand(14, 5) < 0.15] = 220
    img[3:6, :] = 180
    m = W.masks(img, window)
    for method in (W.CA, W.GO, W.SO, W.OS):
        if method in (W.GO, W.SO) and window["train_range"] == 0:
            continue
        want = np.array([[W.cell(img, i, c, dict(window, method=method)) for c in range(5)] for i in range(14)])
        assert np.array_equal(m[method], want), method
    assert any(m[k].any() for k in m)


def test_ca_without_an_azimuth_window_is_the_one_dimensional_detector():
    imgs = synthetic(2, 120, 9, seed=4)
    imgs = np.concatenate([imgs, np.zeros_like(imgs[:1]), np.full_like(imgs[:1], 255)])
    for G, T, scale, mi, mb in ((2, 16, 3.0, 1, 0), (0, 1, 1.5, 0, 5), (5, 200, 2.0, 1, 0)):
        for img in imgs:
            got = W.masks(img, dict(guard_range=G, train_range=T, guard_azimuth=0, train_azimuth=0, scale=scale, min_intensity=mi, min_bin=mb))[W.CA]
            want = detect_ref.cfar_mask(img, G, T, mi, mb, scale)
            assert np.array_equal(got, want)
    assert want.shape == (120, 9)


def test_os_at_the_extreme_ranks_is_the_window_maximum_and_minimum():
    img = synthetic(1, 60, 11, seed=8)[0]
    w = dict(guard_range=1, train_range=3, guard_azimuth=1, train_azimuth=1, scale=1.25, min_intensity=0)
    z = img.astype(np.int64)
    N, A = z.shape
    hi, lo = np.zeros_like(z), np.zeros_like(z)
    for i in range(N):
        for c in range(A):
            t = [z[b, (c + dc) % A] for b in range(max(0, i - 4), min(N, i + 5)) for dc in range(-2, 3) if not (abs(b - i) <= 1 and abs(dc) <= 1)]
            hi[i, c], lo[i, c] = max(t), min(t)
    f32 = np.float32
    assert np.array_equal(W.masks(img, dict(w, rank_permille=1000))[W.OS], z.astype(f32) > f32(1.25) * hi.astype(f32))
    assert np.array_equal(W.masks(img, dict(w, rank_permille=1))[W.OS], z.astype(f32) > f32(1.25) * lo.astype(f32))


def test_the_wall_scene():
    """a wall 12 bins thick across every column: the one-dimensional CA-CFAR finds none of its 444 cells (the wall trains its own
    threshold), OS over the same range window widened by a 1-guard, 2-training azimuth window at rank 500 finds all of them and
    nothing else"""
    img, wall = W.wall_scene()
    assert wall.sum() == 444
    one_d = detect_ref.cfar_mask(img, 2, 16, 1, 0, 4.0)
    assert not (one_d & wall).any()
    os_mask = W.masks(img, dict(guard_range=2, train_range=16, guard_azimuth=1, train_azimuth=2, rank_permille=500, scale=4.0))[W.OS]
    assert np.array_equal(os_mask, wall)
    ca3 = W.masks(img, dict(guard_range=2, train_range=16, guard_azimuth=1, train_azimuth=2, scale=3.0))[W.CA]
    assert (wall & ~ca3).sum() == 323


def test_threshold_table_is_equivalent_to_the_rank_test():
    """what the OS kernel counts against: thr[z] = the largest u with scale * (float)u < (float)z, or -1.  For every z, every v and
    every scale, (float)z > scale * (float)v iff v <= thr[z]; so 'the r-th smallest training value passes' is 'at least r training
    values are <= thr[z]'."""
    f32 = np.float32
    u = np.arange(256, dtype=f32)
    z = np.arange(256, dtype=f32)
    denormal = float(np.float32(1e-40))
    assert 0.0 < denormal < np.finfo(np.float32).tiny
    for scale in (0.0, denormal, 1.0 / 3.0, 1.0, 3.0, 255.0, 1e30):
        with np.errstate(over="ignore", under="ignore"):
            prod = f32(scale) * u                                               # [u]
        passes = z[:, None] > prod[None, :]                                      # [z][v]: the plain test
        assert np.all(passes[:, :-1] >= passes[:, 1:])                           # monotone in v: the passing values are a prefix
        thr = passes.sum(axis=1).astype(np.int64) - 1                            # the largest passing u, -1 if none
        assert np.array_equal(passes, np.arange(256)[None, :] <= thr[:, None])
    # and with the counts: a window of values, every rank
    rs = np.random.RandomState(2)
    for scale in (1.0 / 3.0, 3.0):
        t = np.sort(rs.randint(0, 256, 37))
        thr = (z[:, None] > (f32(scale) * u)[None, :]).sum(axis=1) - 1
        for zz in range(0, 256, 5):
            for r in range(1, 38):
                assert bool(f32(zz) > f32(scale) * f32(t[r - 1])) == bool((t <= thr[zz]).sum() >= r)


def test_radar_facade_has_the_window_calls():
    assert callable(radar.RadarHIP.detectWindow)
    import inspect
    assert "window" in inspect.signature(radar.RadarHIP.simulatePointClouds).parameters


# ---- kernels ------------------------------------------------------------------------------------------------------------------
def test_window_kernels_use_no_scratch_and_no_atomics():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-window"], capture_output=True, text=True, timeout=600)
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
    assert len([n for n in rows if "k_windowIL" in n]) == 8                  # 4 methods x count / emit
    for name, u in rows.items():
        assert u["scratch"] == 0 and u["lds"] <= 2048, (name, u)             # static LDS; the staged step is dynamic
    src = open(os.path.join(CSRC, "rr_window.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code and "k_detect_scan" not in code and "launch_detect_scan" in code


def test_window_source_is_in_the_library_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rr_window.hip" in src
    assert re.search(r"^resource-usage-window:", mk, re.M)
