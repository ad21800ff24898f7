"""The likelihood field without a GPU: the two-pass construction of the distance transform equals the definition (the minimum over the list of
occupied cells) on every grid, map and saturation of the GPU tests, and scipy's transform where scipy is installed; the numpy restatement
(tests/field_ref.py) gives hand-worked answers; the ABI version has not moved and the tile sizes are sane (names, prototypes and the two structs'
layouts: tests/test_abi.py); native.pose_lattice builds what it says; the closed loop's figure is measured on the oracle's images; the wrappers
refuse bad arguments before any call into the library; and the kernels of rr_field.hip use no scratch memory."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import detect_ref
import field_ref as F
import icp_ref
from common import golden_beams, mats_tuple
from radarays_ros_amd import native, params, radar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radarays_ros_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "radarays_mi355.h")
NEW = ["rr_rasterize_points_device", "rr_rasterize_points", "rr_distance_field_device", "rr_distance_field", "rr_score_poses_device",
       "rr_score_poses", "rr_field_tile_sizes"]


# ---- the transform: the construction against the definition -----------------------------------------------------------------
def _grids():
    return F.grid_list(native.field_tile_sizes()[2])


@pytest.mark.parametrize("case", range(8))
def test_the_two_pass_construction_is_the_exact_minimum(case):
    W, H = _grids()[case]
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    for name, occ in F.map_list(W, H).items():
        for md in F.MAX_DISTS:
            cfg = F.grid_cfg(W, H, md)
            got = F.distance_field(occ, cfg)
            assert got.dtype == np.uint16 and got.shape == (H, W)
            assert np.array_equal(got, F.distance_field_brute(occ, cfg)), (W, H, name, md)
            if ndimage is not None and occ.any():
                edt = ndimage.distance_transform_edt(occ == 0)
                assert np.array_equal(got, np.minimum(md * md, np.rint(edt ** 2)).astype(np.uint16)), (W, H, name, md)
            if not occ.any():
                assert np.all(got == md * md)


def test_scipy_agrees_where_it_is_installed():
    ndimage = pytest.importorskip("scipy.ndimage")
    occ = F.map_list(33, 65)["random1"]
    cfg = F.grid_cfg(33, 65, 255)
    want = np.minimum(255 * 255, np.rint(ndimage.distance_transform_edt(occ == 0) ** 2)).astype(np.uint16)
    assert np.array_equal(F.distance_field(occ, cfg), want)


def test_the_saturation_ring_of_a_lone_cell():
    occ = np.zeros((65, 33), np.uint8)
    occ[30, 16] = 1
    got = F.distance_field(occ, F.grid_cfg(33, 65, 3)).astype(np.int64)
    iy, ix = np.mgrid[0:65, 0:33]
    d2 = (iy - 30) ** 2 + (ix - 16) ** 2
    assert np.array_equal(got, np.minimum(9, d2))
    assert sorted(set(got.ravel())) == [0, 1, 2, 4, 5, 8, 9]         # every squared distance below the cap, and the cap
    assert got[30, 19] == 9 and got[32, 18] == 8 and got[33, 16] == 9 and got[30, 20] == 9


def test_threshold_decides_what_is_occupied():
    occ = np.zeros((5, 12), np.uint8)
    occ[2, ::2] = (0, 1, 127, 128, 254, 255)
    cfg = F.grid_cfg(12, 5, 7)
    for th, first in ((1, 2), (128, 6), (255, 10)):
        got = F.distance_field(occ, cfg, th)
        assert np.array_equal(got, F.distance_field_brute(occ, cfg, th))
        assert list(np.nonzero(got[2] == 0)[0]) == list(range(first, 12, 2))


# ---- the restatement on hand-worked cases -----------------------------------------------------------------------------------
def test_the_cell_rule_on_edges_and_outside():
    cfg = native.field_config(4, 3, 0.5, -1.0, -0.5)
    x = np.float32([-1.0, -0.5, 0.99, 1.0, -1.0001, 0.0, 0.0, 0.0, np.nan, np.inf, -np.inf])
    y = np.float32([-0.5, 0.0, 0.99, 0.0, 0.0, 1.0, 0.9999, -0.51, 0.0, 0.0, 0.0])
    inside, index = F.cells(x, y, cfg)
    assert list(inside) == [True, True, True, False, False, False, True, False, False, False, False]
    assert list(index[inside]) == [0, 1 * 4 + 1, 2 * 4 + 3, 2 * 4 + 2]
    occ = F.rasterize([np.stack([x, y], -1)], cfg)
    assert occ.sum() == 4 and occ[0, 0] == occ[1, 1] == occ[2, 3] == occ[2, 2] == 1


def test_rasterize_accumulates_and_applies_the_state():
    cfg = native.field_config(8, 8, 1.0, -4.0, -4.0)
    a, b = np.float32([[1.5, 0.5]]), np.float32([[-2.5, -3.5], [100.0, 0.0]])
    both = F.rasterize([a, b], cfg)
    assert np.array_equal(F.rasterize([b], cfg, occ=F.rasterize([a], cfg)), both) and both.sum() == 2
    turned = F.rasterize([a], cfg, native.se2_states(math.pi / 2))    # c rounds to 6e-17, not 0: (x, y) -> (-y, x) up to that
    assert turned[4 + 1, 4 - 1] == 1 and turned.sum() == 1
    exact = F.rasterize([a], cfg, np.array([[0.0, 1.0, 0.25, 0.0]]))  # the 90-degree state itself, and a shift
    assert exact[4 + 1, 4 - 1] == 1 and exact.sum() == 1
    assert F.rasterize([np.float32([[1.5, 0.5], [2.5, 0.5]])], cfg, max_points=1).sum() == 1


def test_score_counts_every_point():
    cfg = native.field_config(8, 8, 1.0, -4.0, -4.0, 5, 1)
    occ = np.zeros((8, 8), np.uint8)
    occ[4, 4] = 1
    fld = F.distance_field(occ, cfg)
    scan = np.float32([[0.5, 0.5], [1.5, 0.5], [2.5, 2.5], [50.0, 0.0], [np.nan, 0.0]])     # d2 = 0, 1, 8, outside, outside
    st = np.float32([[1, 0, 0, 0], [1, 0, 100, 0], [np.nan, 0, 0, 0], [1, 0, -1, 0]])
    r = F.score(scan, st, fld, cfg)
    assert r.dtype == native.FIELD_DTYPE
    assert (r[0]["sum_d2"], r[0]["n_in"], r[0]["n_hit"]) == (0 + 1 + 8 + 25 + 25, 3, 2)
    assert (r[1]["sum_d2"], r[1]["n_in"], r[1]["n_hit"]) == (5 * 25, 0, 0) == (r[2]["sum_d2"], r[2]["n_in"], r[2]["n_hit"])
    assert (r[3]["sum_d2"], r[3]["n_in"], r[3]["n_hit"]) == (1 + 0 + 5 + 25 + 25, 3, 2)
    assert np.all(F.score(scan[:0], st, fld, cfg).view(np.uint8) == 0)
    assert F.score(scan, st[:1], fld, cfg, max_points=2)[0]["sum_d2"] == 1


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_field_entry_points_are_declared_and_exported(native_lib):
    """(names, argument types and struct layouts: tests/test_abi.py, for the whole header)"""
    header = open(HEADER).read()
    assert "#define RR_ABI_VERSION 7" in header
    assert native_lib.lib().rr_abi_version() == 7
    points_tile, hyps, row_tile = native_lib.field_tile_sizes()
    assert points_tile >= 64 and points_tile % 64 == 0 and hyps >= 1 and row_tile >= 1


def test_pose_lattice_shapes_and_its_centre_node():
    st, xyz = native.pose_lattice((1.5, -2.0, 0.3), 1.0, 0.25, math.radians(4.0), math.radians(1.0))
    assert st.shape == (729, 4) and st.dtype == np.float32 and xyz.shape == (729, 3) and xyz.dtype == np.float64
    mid = 729 // 2
    assert tuple(xyz[mid]) == (1.5, -2.0, 0.3)
    assert tuple(st[mid]) == (np.float32(math.cos(0.3)), np.float32(math.sin(0.3)), np.float32(1.5), np.float32(-2.0))
    assert np.allclose(xyz.min(0), (0.5, -3.0, 0.3 - math.radians(4.0))) and np.allclose(xyz.max(0), (2.5, -1.0, 0.3 + math.radians(4.0)))
    assert np.array_equal(st[:, 0], np.cos(xyz[:, 2]).astype(np.float32)) and np.array_equal(st[:, 2], xyz[:, 0].astype(np.float32))
    assert xyz[1, 2] > xyz[0, 2] and xyz[1, 0] == xyz[0, 0]          # yaw runs fastest, x slowest
    one, node = native.pose_lattice((0.0, 0.0, 0.0), 0.0, 1.0, 0.0, 1.0)
    assert one.shape == (1, 4) and tuple(one[0]) == (1.0, 0.0, 0.0, 0.0) and tuple(node[0]) == (0.0, 0.0, 0.0)
    for bad in (dict(step_xy=0.0), dict(step_yaw=-1.0), dict(half_extent_xy=float("nan")), dict(center_xy_yaw=(0.0, 0.0))):
        kw = dict(center_xy_yaw=(0.0, 0.0, 0.0), half_extent_xy=1.0, step_xy=0.5, half_yaw=0.1, step_yaw=0.1)
        kw.update(bad)
        with pytest.raises(ValueError):
            native.pose_lattice(**kw)
    with pytest.raises(ValueError):
        native.pose_lattice((0.0, 0.0, 0.0), 100.0, 0.01, 1.0, 0.001)     # more than 2^22 nodes


# ---- the closed loop's figure, measured here on the oracle's images ---------------------------------------------------------------
def loop_clouds():
    from oracle import oracle
    s, cfg = icp_ref.loop_scene(), icp_ref.loop_cfg()
    sc = oracle.Scene(s["verts"], s["faces"], s["face_object_id"], use_bvh=0)
    theta_inc = np.float32(-2 * np.pi / icp_ref.LOOP_ANGLES)
    clouds = []
    for pose in (icp_ref.LOOP_A, icp_ref.LOOP_B):
        img = oracle.simulate(sc, mats_tuple(params.kaist_materials()), s["object_materials"], cfg, golden_beams(icp_ref.LOOP_SAMPLES),
                              icp_ref.loop_pose(pose), n_angles=icp_ref.LOOP_ANGLES, want_f32=False)[0]
        clouds.append(detect_ref.detect_frame(img, theta_min=0.0, theta_inc=theta_inc, resolution=cfg.resolution, **icp_ref.LOOP_DET)[0])
    return clouds


def test_closed_loop_figure_on_the_oracles_images():
    a, b = loop_clouds()
    assert len(a) >= 100 and len(b) >= 100
    cfg = F.loop_field_cfg()
    occ = F.rasterize([a], cfg, F.loop_map_state())
    fld = F.distance_field(occ, cfg)
    assert np.array_equal(fld, F.distance_field_brute(occ, cfg))
    states, xyz = F.loop_lattice()
    assert len(states) == 729
    rec = F.score(b, states, fld, cfg)
    best = int(np.argmin(rec["sum_d2"]))
    centre = len(states) // 2
    ex, ey, eyaw = F.loop_errors(xyz[best])
    print("closed loop on the oracle's images: %d cells occupied; argmin node (%.2f m, %.2f m, %.1f deg) at sum_d2 %d (centre node %d), off the "
          "truth by %.3f m, %.3f m, %.3f deg" % (occ.sum(), xyz[best][0], xyz[best][1], math.degrees(xyz[best][2]), rec["sum_d2"][best],
                                               rec["sum_d2"][centre], ex, ey, math.degrees(eyaw)))
    assert np.count_nonzero(rec["sum_d2"] == rec["sum_d2"][best]) == 1        # the argmin is unique
    assert rec["sum_d2"][best] < rec["sum_d2"][centre]                        # ... beats the identity guess
    assert np.all(rec["n_in"] == len(b))                                      # ... and no hypothesis throws a point off the grid
    # near the truth: within one lattice step in each of x, y and yaw
    assert ex <= F.LOOP_STEP_XY and ey <= F.LOOP_STEP_XY and eyaw <= F.LOOP_STEP_YAW
    # the constants are what is measured here
    assert abs(ex - F.LOOP_X_MEASURED) <= 1e-9 and abs(ey - F.LOOP_Y_MEASURED) <= 1e-9 and abs(eyaw - F.LOOP_YAW_MEASURED) <= 1e-9


# ---- wrappers refuse before the library -------------------------------------------------------------------------------------------
def _unopened(n_cells=64, n_angles=16):
    o = native.Context.__new__(native.Context)
    o._h = None
    o._L = None
    o.cfg = params.RadarModelConfig(n_cells=n_cells)
    o.n_angles = n_angles
    return o


def test_field_config_is_range_checked():
    g = native.field_config(4096, 1, 0.25, -3.0, 7.5, 255, 255)
    assert (g.width, g.height, g.cell, g.x0, g.y0, g.max_dist, g.gate, g.reserved_) == (4096, 1, 0.25, -3.0, 7.5, 255, 255, 0)
    good = dict(width=8, height=8, cell=0.5, x0=0.0, y0=0.0, max_dist=10, gate=3)
    for bad in (dict(width=0), dict(width=4097), dict(height=0), dict(height=4097), dict(height=2.0), dict(cell=0.0), dict(cell=-1.0),
                dict(cell=float("nan")), dict(cell=float("inf")), dict(cell=1e-50), dict(x0=float("nan")), dict(y0=float("inf")), dict(x0=1e39),
                dict(max_dist=0), dict(max_dist=256), dict(gate=-1), dict(gate=11), dict(gate=True), dict(cell="wide")):
        with pytest.raises(ValueError):
            native.field_config(**dict(good, **bad))


def test_wrappers_refuse_bad_arguments_before_the_library():
    o = _unopened()
    g = native.field_config(8, 8, 0.5, 0.0, 0.0, 4, 1)
    pts = [F.points_of(np.zeros((3, 2))), F.points_of(np.zeros((1, 2)))]
    offs = np.zeros((2, 17), np.uint32)
    offs[:, -1] = (3, 1)
    for bad_pts, bad_offs in (([np.zeros(3, np.float32)] * 2, offs), (pts, offs[:1]), (pts, offs.astype(np.int32)), ([], offs), (pts[:1] * 2, offs)):
        with pytest.raises(ValueError):
            o.rasterize_points(bad_pts, bad_offs, g)
    for bad_states in (np.zeros((1, 4)), np.zeros((2, 3)), np.zeros((2, 4), complex)):
        with pytest.raises(ValueError):
            o.rasterize_points(pts, offs, g, states=bad_states)
    with pytest.raises(ValueError):
        o.rasterize_points(pts, offs, g, occ=np.zeros((8, 9), np.uint8))
    with pytest.raises(ValueError):
        o.rasterize_points(pts, offs, "grid")
    for occ in (np.zeros((8, 8), np.uint16), np.zeros((7, 8), np.uint8)):
        with pytest.raises(ValueError):
            o.distance_field(occ, g)
    for th in (0, 256, 1.5, True):
        with pytest.raises(ValueError):
            o.distance_field(np.zeros((8, 8), np.uint8), g, threshold=th)
        with pytest.raises(ValueError):
            o.distance_field_device(1, g, 2, threshold=th)
    for args in ((None, g, 2), (1, g, None), (1, g, 1)):
        with pytest.raises(ValueError):
            o.distance_field_device(*args)
    fld, st = np.zeros((8, 8), np.uint16), np.zeros((2, 4), np.float32)
    for bad in ((pts[0], st[:0], fld), (pts[0], np.zeros((2, 3), np.float32), fld), (pts[0], st, fld.astype(np.uint8)), (np.zeros((3, 2)), st, fld),
                (pts[0], st, np.zeros((8, 7), np.uint16))):
        with pytest.raises(ValueError):
            o.score_poses(*bad, g)
    for n_hyp in (0, (1 << 22) + 1, -1):
        with pytest.raises(ValueError):
            o.score_poses_device(1, 1, 4, 1, n_hyp, 1, g, 1)
    for mp in (-1, 65537):
        with pytest.raises(ValueError):
            o.score_poses_device(1, 1, mp, 1, 2, 1, g, 1)
        with pytest.raises(ValueError):
            o.rasterize_points_device(1, 1, 2, mp, g, 1)
    for n in (0, 65536):
        with pytest.raises(ValueError):
            o.rasterize_points_device(1, 1, n, 4, g, 1)
    for args in ((None, 1, 4, 1, 2, 1, g, 1), (1, None, 4, 1, 2, 1, g, 1), (1, 1, 4, None, 2, 1, g, 1), (1, 1, 4, 1, 2, None, g, 1),
                 (1, 1, 4, 1, 2, 1, g, None)):
        with pytest.raises(ValueError):
            o.score_poses_device(*args)
    for args in ((None, 1, 2, 4, g, 1), (1, None, 2, 4, g, 1), (1, 1, 2, 4, g, None)):
        with pytest.raises(ValueError):
            o.rasterize_points_device(*args)
    with pytest.raises(native.RRError, match="rr_set_config"):
        u = _unopened(); u.cfg = None; u.rasterize_points(pts, offs, g)


def test_the_facades_have_the_field_calls():
    assert callable(radar.RadarHIP.buildLikelihoodField) and callable(radar.RadarHIP.scorePoses)
    assert "sensor frame into the map frame" in radar.RadarHIP.scorePoses.__doc__
    hpp = open(os.path.join(ROOT, "include", "radarays_ros_amd", "RadarHIP.hpp")).read()
    for n in ("buildLikelihoodField", "scorePoses", "rr_field_rec", "rr_field_config"):
        assert n in hpp, n
    marshal = open(os.path.join(ROOT, "include", "radarays_ros_amd", "marshal.hpp")).read()
    assert "rr_score_poses" in marshal and "rr_rasterize_points" in marshal and "rr_distance_field" in marshal


# ---- kernels ------------------------------------------------------------------------------------------------------------------------
def test_field_kernels_use_no_scratch(native_lib):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-field"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    rows, cur = {}, None
    for line in (r.stdout + r.stderr).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        for key, name in ((r"ScratchSize \[bytes/lane\]", "scratch"), (r"LDS Size \[bytes/block\]", "lds"), (r"VGPRs", "vgprs")):
            m = re.search(r"remark:\s+" + key + r": (\d+)", line)
            if m and cur is not None:
                cur[name] = int(m.group(1))
    names = " ".join(rows)
    for k in ("k_field_raster", "k_field_columns", "k_field_rows", "k_field_score"):
        assert k in names, (k, sorted(rows))
    for name, u in rows.items():
        assert u["scratch"] == 0, (name, u)
        # the staged row of the row pass: 4096 cells between two aprons of 255, a u16 each; nothing anywhere else
        assert u["lds"] == (2 * (4096 + 2 * 255) if "k_field_rows" in name else 0), (name, u)
        assert u["vgprs"] <= 64, (name, u)                                               # eight waves per SIMD


def test_field_source_is_in_the_library_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rr_field.hip" in src
    assert re.search(r"^resource-usage-field:", mk, re.M)
    launch = open(os.path.join(CSRC, "rr_launch.h")).read()
    for name in ("field_tile_sizes", "launch_field_raster", "launch_distance_field", "launch_field_score"):
        assert len(re.findall(r"\b%s\(" % name, launch)) == 1, name
    images = open(os.path.join(CSRC, "rr_images.hip")).read()
    for n in NEW:
        assert re.search(r"^(int|void) %s\(" % n, images, re.M), n
