"""Sweep compensation without a GPU: the ABI version has not moved (names, prototypes and the layout of
rr_sweep_rec: tests/test_abi.py), sweep_poses and the numpy restatement (tests/deskew_ref.py) give hand-worked answers, the Python wrappers refuse bad
shapes before any call into the library, the inputs of the GPU comparison stay clear of rounding boundaries, and the kernels of
rr_deskew.hip use no scratch."""
import os
import re
import subprocess

import numpy as np
import pytest

import deskew_ref as R
from radarays_ros_amd import native, params, radar, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radarays_ros_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "radarays_mi355.h")
IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)


def test_sweep_entry_points_are_declared_and_exported(native_lib):
    """(names, argument types and struct layouts: tests/test_abi.py, for the whole header)"""
    header = open(HEADER).read()
    assert "#define RR_ABI_VERSION 7" in header
    assert native_lib.lib().rr_abi_version() == 7


# ---- sweep_poses on hand-worked twists --------------------------------------------------------------------------------
def yaw_of(q):
    return 2.0 * np.arctan2(q[..., 2].astype(np.float64), q[..., 3].astype(np.float64))


def test_sweep_poses_zero_twist_copies_the_reference_pose():
    pose = scenes.yaw_pose(1.0, -2.0, 0.5, 0.7)
    table, vel = scenes.sweep_poses(pose, np.zeros(6), 0.25, 37, 11)
    assert table.shape == (37, 7) and table.dtype == np.float32
    assert np.allclose(table, np.tile(pose, (37, 1)), atol=1e-7) and np.all(vel == 0)


def test_sweep_poses_pure_yaw_rate_grows_the_yaw_linearly():
    pose = scenes.yaw_pose(1.0, -2.0, 0.5, 0.3)
    table, vel = scenes.sweep_poses(pose, [0, 0, 0, 0, 0, 0.8], 0.5, 40, 10)
    want = 0.3 + 0.8 * (np.arange(40) - 10) / 40 * 0.5
    assert np.allclose(yaw_of(table[:, :4]), want, atol=1e-6)
    assert np.allclose(table[:, 4:], pose[4:], atol=1e-7) and np.all(vel == 0)
    assert np.allclose(table[10], pose, atol=1e-7)                  # the reference azimuth holds the reference pose


def test_sweep_poses_pure_forward_speed_moves_along_the_heading():
    yaw = 0.6
    pose = scenes.yaw_pose(1.0, -2.0, 0.5, yaw)
    table, vel = scenes.sweep_poses(pose, [20.0, 0, 0, 0, 0, 0], 0.25, 64, 0)
    heading = np.array([np.cos(yaw), np.sin(yaw), 0.0])
    want = pose[4:] + 20.0 * (np.arange(64) / 64 * 0.25)[:, None] * heading
    assert np.allclose(table[:, 4:], want, atol=1e-5)
    assert np.allclose(table[:, :4], pose[:4], atol=1e-7)
    assert np.allclose(vel, 20.0 * heading, atol=1e-5)


def test_sweep_poses_arc_of_a_turning_vehicle():
    """v = 2 m/s with 1 rad/s for pi / 2 s from the origin: a quarter of the circle of radius 2 about (0, 2)"""
    table, vel = scenes.sweep_poses(IDENT, [2.0, 0, 0, 0, 0, 1.0], np.pi / 2 * 8 / 7, 8, 0)
    assert np.allclose(table[7, 4:], [2.0, 2.0, 0.0], atol=1e-6) and abs(yaw_of(table[7, :4]) - np.pi / 2) < 1e-6


# ---- the restatement on hand-worked tables ----------------------------------------------------------------------------
def points(xyz, column, bin_):
    p = np.zeros(len(xyz), native.POINT_DTYPE)
    p["x"], p["y"], p["z"] = np.asarray(xyz, np.float32).T
    p["column"], p["bin"], p["intensity"] = column, bin_, 9.0
    return p


def test_identity_table_leaves_points_unchanged():
    res = 0.5
    p = points([[1.25, 0, 0], [0, 3.25, 0]], [0, 2], [2, 6])
    out = R.compensate_points(p, native.identity_sweep_table(1, 4)[0], resolution=res)
    assert out.tobytes() == p.tobytes()


def test_translation_table_moves_a_point_and_dr_shortens_it():
    t = native.identity_sweep_table(1, 4)[0]
    t["t"][1] = (1.0, -2.0, 0.5)
    p = points([[1.25, 0, 0], [1.25, 0, 0]], [1, 0], [2, 2])           # scroll 0: column = azimuth
    out = R.compensate_points(p, t, resolution=0.5)
    assert [out["x"][0], out["y"][0], out["z"][0]] == [2.25, -2.0, 0.5] and out["x"][1] == 1.25
    t["dr"][0] = 0.25                                                 # bin 2 at 1.25 m: rc = 1.0
    out = R.compensate_points(p, t, resolution=0.5)
    assert out["x"][1] == 1.0 and list(out["column"]) == [1, 0] and list(out["bin"]) == [2, 2] and np.all(out["intensity"] == 9.0)
    t["dr"][0] = 1.25                                                 # rc = 0: no such range
    assert np.isnan(R.compensate_points(p, t, resolution=0.5)["x"][1])
    # the column's azimuth goes through the scroll: column 1 with scroll 1 is azimuth 0
    assert np.isnan(R.compensate_points(p, t, scroll=1, resolution=0.5)["x"][0])


def test_quarter_turn_maps_x_to_y():
    t = native.identity_sweep_table(1, 4)[0]
    t["q"][:] = (0.0, 0.0, np.sin(np.pi / 4), np.cos(np.pi / 4))
    out = R.compensate_points(points([[1.25, 0, 0]], [3], [2]), t, resolution=0.5)
    assert np.allclose([out["x"][0], out["y"][0], out["z"][0]], [0.0, 1.25, 0.0], atol=1e-6)
    # the table of the restatement: a sensor yawed by 90 degrees against its reference, 2 m ahead of it
    tab = R.sweep_table(np.tile(scenes.yaw_pose(2.0, 0.0, 0.0, np.pi / 2), (1, 4, 1)), IDENT[None], [[3.0, 0.0, 0.0]], 0.1,
                        theta_min=0.0, theta_inc=-np.pi / 2)
    assert np.allclose(tab["q"][0, 0], t["q"][0], atol=1e-6) and np.allclose(tab["t"][0, 0], [2.0, 0.0, 0.0], atol=1e-6)
    # azimuth 0 looks along the sensor's +x = the map's +y: no range rate; azimuth 3 (yaw -3 pi / 2 = +y of the sensor = -x of the map)
    # recedes from a world it drives away from at 3 m/s: v_r = +3, dr = +0.3
    assert np.allclose(tab["dr"][0], [0.0, -0.3, 0.0, 0.3], atol=1e-6)
    assert np.all(R.sweep_table(np.tile(IDENT, (1, 4, 1)), IDENT[None], [[3.0, 0, 0]], 0.0)["dr"] == 0)
    assert np.all(R.sweep_table(np.tile(IDENT, (1, 4, 1)), IDENT[None], None, 0.1)["dr"] == 0)


def test_cartesian_restatement_identity_is_the_plain_conversion():
    import detect_ref
    img = np.random.RandomState(3).randint(0, 256, (96, 37)).astype(np.uint8)
    g = dict(scroll=5, theta_min=0.1, theta_inc=-2 * np.pi / 37, resolution=0.0595238)
    for bilinear in (False, True):
        want = detect_ref.cartesian(img, 33, 0.35, bilinear, **g)
        for it in (1, 3):
            got = R.cartesian_sweep(img, native.identity_sweep_table(1, 37)[0], 33, 0.35, bilinear, it, **g)
            assert np.array_equal(got, want)


def test_cartesian_restatement_undoes_a_forward_offset():
    """every azimuth measured 2 m ahead of the reference pose: the ring at bin b of the polar image lands 2 m further ahead"""
    img = np.zeros((50, 400), np.uint8)
    img[10] = 200                                                     # a ring at 10.5 m
    t = native.identity_sweep_table(1, 400)[0]
    t["t"][:, 0] = 2.0
    out = R.cartesian_sweep(img, t, 41, 1.0, False, 2, resolution=1.0)
    col = out[:, 20]                                                  # the centre column: x = 20 - i
    # bin 10 is read where v = rho - 0.5 rounds (half to even) to 10: rho = |x - 2| = 10 and 11, so x = 12, 13 ahead and -8, -9 behind
    assert list(np.nonzero(col)[0]) == [7, 8, 28, 29]
    t["dr"][:] = 3.0                                                  # the ring was drawn 3 m too far out: its true range is 7.5 m
    col = R.cartesian_sweep(img, t, 41, 1.0, False, 2, resolution=1.0)[:, 20]
    assert list(np.nonzero(col)[0]) == [10, 11, 25, 26]               # |x - 2| + 3 = 10 and 11: x = 9, 10 and -5, -6


def test_the_cartesian_inputs_stay_clear_of_rounding_boundaries():
    """the float32 restatement against itself in float64 on the inputs of the GPU comparison: inside the comparison's own criterion"""
    res = params.kaist_preset().resolution
    tables = {}
    for n_frames, n_angles, width, bilinear, iterations in R.CART_CASES:
        key = (n_frames, n_angles, bilinear)
        if key not in tables:
            imgs, az, ref, vel = R.cart_case(n_frames, n_angles, bilinear, res)
            g = dict(theta_min=R.CART_THETA_MIN, theta_inc=np.float32(-2 * np.pi / n_angles))
            tables[key] = (imgs, R.sweep_table(az, ref, vel, R.CART_GAIN, **g), g)
        imgs, table, g = tables[key]
        ps = R.cart_pixel_size(width, res)
        for f in range(n_frames):
            a = R.cartesian_sweep(imgs[f], table[f], width, ps, bilinear, iterations, scroll=R.CART_SCROLL, resolution=res, **g)
            b = R.cartesian_sweep(imgs[f], table[f], width, ps, bilinear, iterations, scroll=R.CART_SCROLL, resolution=res, dtype=np.float64, **g)
            d = np.abs(a.astype(int) - b)
            assert d.max() <= 1 and np.mean(d > 0) <= 1e-3, (n_frames, n_angles, width, bilinear, iterations, f, d.max(), np.mean(d > 0))
            assert a.any()


# ---- wrappers refuse before the library -------------------------------------------------------------------------------
def _unopened(n_cells=64, n_angles=16):
    o = native.Context.__new__(native.Context)
    o._h = None
    o._L = None
    o.cfg = params.RadarModelConfig(n_cells=n_cells)
    o.n_angles = n_angles
    return o


def test_wrappers_refuse_bad_tables_and_poses_before_the_library():
    o = _unopened()
    az, ref = np.tile(IDENT, (2, 16, 1)), np.tile(IDENT, (2, 1))
    for bad_az, bad_ref, vel, gain in ((az[:, :15], ref, None, 0.0), (az, ref[:1], None, 0.0), (az[..., :6], ref, None, 0.0),
                                       (az, ref, np.zeros((3, 3)), 0.1), (az, ref, np.zeros((2, 2)), 0.1), (az, ref, None, float("nan")),
                                       (az, ref, None, float("inf")), (az, ref, None, "fast"), (az.astype(complex), ref, None, 0.0)):
        with pytest.raises(ValueError):
            o.sweep_table(bad_az, bad_ref, vel, gain)
    img = np.zeros((2, 64, 16), np.uint8)
    good = native.identity_sweep_table(2, 16)
    for bad in (good[:1], good[:, :15], np.zeros((2, 16), np.float32), good.view(np.uint8)):
        with pytest.raises(ValueError):
            o.polar_to_cartesian_sweep(img, bad, 32, 0.5)
        with pytest.raises(ValueError):
            o.compensate_points([np.zeros(0, native.POINT_DTYPE)] * 2, np.zeros((2, 17), np.uint32), bad)
    for it in (0, 9, 2.5, True):
        with pytest.raises(ValueError):
            o.polar_to_cartesian_sweep(img, good, 32, 0.5, iterations=it)
        with pytest.raises(ValueError):
            o.polar_to_cartesian_sweep_device(1, 2, 32, 0.5, 1, 1, iterations=it)
    for w, ps in ((0, 1.0), (8193, 1.0), (16, 0.0), (16, float("nan"))):
        with pytest.raises(ValueError):
            o.polar_to_cartesian_sweep(img, good, w, ps)
    with pytest.raises(ValueError):
        o.polar_to_cartesian_sweep(img.astype(np.float32), good, 32, 0.5)
    pts = [np.zeros(3, native.POINT_DTYPE), np.zeros(0, native.POINT_DTYPE)]
    offs = np.zeros((2, 17), np.uint32)
    offs[0, -1] = 3
    for bad_pts, bad_offs in (([np.zeros(3, np.float32)] * 2, offs), (pts, offs[:1]), (pts, offs.astype(np.int32)), (pts[:1] * 2, offs), ([], offs)):
        with pytest.raises(ValueError):
            o.compensate_points(bad_pts, bad_offs, good)
    for n in (0, 65536, -1):
        with pytest.raises(ValueError):
            o.sweep_table_device(1, 1, n, 1)
        with pytest.raises(ValueError):
            o.compensate_points_device(1, 1, n, 4, 1)
        with pytest.raises(ValueError):
            o.polar_to_cartesian_sweep_device(1, n, 16, 1.0, 1, 1)
    for args in ((None, 1, 1, 1), (1, None, 1, 1), (1, 1, 1, None)):
        with pytest.raises(ValueError):
            o.sweep_table_device(*args)
    with pytest.raises(ValueError):
        o.compensate_points_device(1, 1, 1, -1, 1)
    with pytest.raises(ValueError):
        o.compensate_points_device(None, 1, 1, 4, 1)
    with pytest.raises(ValueError):
        _unopened(4, 2049).polar_to_cartesian_sweep_device(1, 1, 16, 1.0, 1, 1)
    with pytest.raises(native.RRError, match="rr_set_config"):
        u = _unopened(); u.cfg = None; u.sweep_table(az, ref)


def test_the_facades_have_the_compensation_calls():
    assert callable(radar.RadarHIP.simulate_sweep)
    hpp = open(os.path.join(ROOT, "include", "radarays_ros_amd", "RadarHIP.hpp")).read()
    for n in ("sweepTable", "compensatePointClouds", "compensatedCartesian", "rr_compensate_points", "rr_polar_to_cartesian_sweep"):
        assert n in hpp, n


# ---- kernels ----------------------------------------------------------------------------------------------------------
def test_deskew_kernels_use_no_scratch():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-deskew"], capture_output=True, text=True, timeout=600)
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
    for k in ("k_sweep_table", "k_compensate_points", "k_cartesian_sweepILi0", "k_cartesian_sweepILi1"):
        assert k in names, (k, sorted(rows))
    for name, u in rows.items():
        assert u["scratch"] == 0 and u["lds"] == 0, (name, u)            # no static LDS; the records are dynamic (<= 64 KB)


def test_deskew_source_is_in_the_library_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rr_deskew.hip" in src
    assert re.search(r"^resource-usage-deskew:", mk, re.M)
