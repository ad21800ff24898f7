"""Occupancy mapping without a GPU: the numpy restatement (tests/occupancy_ref.py) holds its profile and hit steps to a brute-force f64 version
and gives hand-worked answers; the ABI version has not moved and the tile sizes are sane (names, prototypes and the struct's layout:
tests/test_abi.py); the wrappers refuse bad arguments before any call into the library; the facades and the marshalling exist and the C++
method compiles; rr_occupancy.hip is in the library build with each launcher declared once; its kernels use no scratch memory; and the
closed loop's three statements hold on the oracle's images with the values tests/occupancy_ref.py records."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import detect_ref
import field_ref as F
import icp_ref
import occupancy_ref as O
from common import golden_beams, mats_tuple
from radarays_ros_amd import native, params, radar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radarays_ros_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "radarays_mi355.h")
NEW = ["rr_occupancy_update_device", "rr_occupancy_update", "rr_occupancy_map_device", "rr_occupancy_map", "rr_occupancy_tile_sizes"]
N_ANGLES, N_CELLS = 16, 64


def synthetic(seed, G, n=3, k_max=3):
    """n scans as rr_detect writes them, every point at the centre of its bin along its azimuth: away from the cell edges of the grids below
    but for an unlucky few, which the callers' grids avoid by their odd cell size"""
    rs = np.random.RandomState(seed)
    clouds, offs = [], []
    for _ in range(n):
        empty = set(rs.choice(G.n_angles, 3, replace=False))
        cols, bins = [], []
        for col in range(G.n_angles):
            k = 0 if col in empty else int(rs.randint(1, k_max + 1))
            cols += [col] * k
            bins += list(np.sort(rs.choice(np.arange(0, G.n_cells), k, replace=False)))
        cols, bins = np.asarray(cols, np.int64), np.asarray(bins, np.int64)
        p = np.zeros(len(cols), native.POINT_DTYPE)
        theta = np.float32(G.theta_min) + ((cols - G.scroll) % G.n_angles).astype(np.float32) * np.float32(G.theta_inc)
        r = ((bins.astype(np.float64) + 0.5) * G.resolution).astype(np.float32)
        p["x"], p["y"], p["column"], p["bin"] = r * np.cos(theta), r * np.sin(theta), cols, bins
        o = np.zeros(G.n_angles + 1, np.uint32)
        o[1:] = np.cumsum(np.bincount(cols, minlength=G.n_angles))
        clouds.append(p)
        offs.append(o)
    return clouds, np.stack(offs)


# ---- the restatement against brute force ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scroll", [0, 5])
def test_profile_and_hits_equal_a_brute_force_f64_version(scroll):
    G = O.polar(N_CELLS, N_ANGLES, scroll, resolution=0.0595238)
    clouds, offs = synthetic(11 + scroll, G)
    cfg = native.field_config(41, 37, 0.2003, -4.1, -3.7)
    states = native.se2_states([0.0, 0.7, -2.0], [0.0, 0.3, -0.5], [0.0, -0.2, 0.4])
    cut = int(offs[0][9]) + 1
    for m in (O.model(3, 1, 0, N_CELLS), O.model(3, 1, 6, N_CELLS), O.model(3, 1, N_CELLS, N_CELLS), O.model(3, 1, 2, 0), O.model(3, 1, 3, 17)):
        for mp in (None, cut, 0):
            got = O.profile(clouds, offs, G, m, mp)
            want = O.profile_brute(clouds, G, m, mp)
            assert got.dtype == np.float32 and np.allclose(got, want, rtol=3e-7, atol=0), (m, mp)      # f32 of an f64 product, squared in f32
            assert np.array_equal(got == 0, want == 0)
    for st in (None, states):
        for mp in (None, cut):
            hits = O.hit_counts(clouds, cfg, st, mp)
            assert np.array_equal(hits, O.hit_counts_brute(clouds, cfg, st, mp))
            assert hits.sum() > 0
    assert O.hit_counts(clouds, cfg, states).sum() == sum(len(c) for c in clouds)          # every point is IN GRID, several share a cell
    assert O.hit_counts(clouds, cfg, states).max() >= 2


def test_the_free_pass_on_a_hand_worked_grid():
    """one scan at the origin of a 5 x 5 grid of 1 m cells, 4 azimuths a quarter turn apart (clockwise), bins of 1 m: azimuth 0 (+x) free for 2
    bins, azimuth 1 (-y) for 1, azimuth 2 (-x) for none, azimuth 3 (+y) empty and free up to max_free_bin = 2"""
    G = O.polar(8, 4, resolution=1.0)
    cfg = native.field_config(5, 5, 1.0, -2.5, -2.5)
    p = np.zeros(3, native.POINT_DTYPE)
    p["column"], p["bin"] = (0, 1, 2), (3, 2, 1)
    p["x"], p["y"] = (3.5, 0.0, -1.5), (0.0, -2.5, 0.0)
    offs = np.uint32([[0, 1, 2, 3, 3]])
    m = O.model(l_hit=5, l_free=2, margin_bins=1, max_free_bin=2)
    free2 = O.profile([p], offs, G, m)
    assert list(free2[0]) == [4.0, 1.0, 0.0, 4.0]
    n_free, a = O.free_counts(free2, cfg, G)
    assert a[2, 4] == 0 and a[0, 2] == 1 and a[2, 0] == 2 and a[4, 2] == 3 and a[2, 2] == 0      # atan2f(0, 0) = 0: azimuth 0
    want = np.zeros((5, 5), np.int64)
    want[2, 2] = want[2, 3] = 1              # +x: rho2 0 and 1 are below 4, rho2 4 is not
    want[3, 2] = 1                           # +y, the empty azimuth: free up to 2 m
    want[3, 3] = 1                           # the diagonal (1, 1): 45 degrees clockwise-negative is u = 3.5 -> rint to even 4 -> azimuth 0; rho2 2 < 4
    want[1, 3] = 1                           # the diagonal (1, -1): u = 0.5 -> rint to even 0 -> azimuth 0 as well
    assert np.array_equal(n_free, want), n_free
    ev = O.update([p], offs, cfg, G, m)
    hit = np.zeros((5, 5), np.int64)
    hit[2, 1] = hit[0, 2] = 1                # (3.5, 0) lies outside the grid
    assert np.array_equal(ev, 5 * hit - 2 * want) and ev.dtype == np.int32
    assert np.array_equal(O.update([p], offs, cfg, G, m, evidence=ev), 2 * ev)
    assert list(O.to_map(np.int32([-300, -128, -1, 0, 1, 127, 300]))) == [0, 0, 127, 128, 129, 255, 255]


def test_fusion_is_a_sum_whatever_the_order():
    G = O.polar(N_CELLS, N_ANGLES, resolution=0.0595238)
    clouds, offs = synthetic(3, G, n=4)
    cfg = native.field_config(21, 19, 0.4, -4.2, -3.8)
    st = native.se2_states([0.1, 1.0, -2.0, 3.0], [0.2, -0.3, 0.0, 0.5], [0.0, 0.4, -0.4, 0.1])
    m = O.model(4, 3, 2, N_CELLS)
    whole = O.update(clouds, offs, cfg, G, m, st)
    parts = sum(O.update(clouds[f:f + 1], offs[f:f + 1], cfg, G, m, st[f:f + 1]).astype(np.int64) for f in range(4))
    assert np.array_equal(whole, parts)
    back = O.update(clouds[:2], offs[:2], cfg, G, m, st[:2], evidence=O.update(clouds[2:], offs[2:], cfg, G, m, st[2:]))
    assert np.array_equal(back, whole) and (whole > 0).any() and (whole < 0).any()


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_occupancy_entry_points_are_declared_and_exported(native_lib):
    header = open(HEADER).read()
    assert "#define RR_ABI_VERSION 7" in header
    assert native_lib.lib().rr_abi_version() == 7
    for n in NEW:
        assert n in native_lib.PROTOTYPES and hasattr(native_lib.lib(), n), n
    group, per_thread, chunk = native_lib.occupancy_tile_sizes()
    assert group >= 64 and per_thread >= 1 and group % (64 * per_thread) == 0 and chunk >= 0
    import ctypes as C
    assert C.sizeof(native_lib.RROccupancyConfig) == 32


# ---- wrappers refuse before the library -------------------------------------------------------------------------------------------------
def _unopened():
    o = native.Context.__new__(native.Context)
    o._h = None
    o._L = None
    o.cfg = params.RadarModelConfig(n_cells=N_CELLS)
    o.n_angles = N_ANGLES
    return o


def test_occupancy_config_is_range_checked():
    c = native.occupancy_config(127, 0, 64, 0, 64)
    assert (c.l_hit, c.l_free, c.margin_bins, c.max_free_bin, list(c.reserved_)) == (127, 0, 64, 0, [0, 0, 0, 0])
    good = dict(l_hit=3, l_free=1, margin_bins=2, max_free_bin=60, n_cells=64)
    for bad in (dict(l_hit=0), dict(l_hit=128), dict(l_hit=1.0), dict(l_free=-1), dict(l_free=128), dict(l_free=True), dict(margin_bins=-1),
                dict(margin_bins=65), dict(max_free_bin=-1), dict(max_free_bin=65), dict(max_free_bin="far"), dict(n_cells=0)):
        with pytest.raises(ValueError):
            native.occupancy_config(**dict(good, **bad))


def test_wrappers_refuse_bad_arguments_before_the_library():
    o = _unopened()
    g = native.field_config(8, 8, 0.5, 0.0, 0.0)
    m = O.model(3, 1, 2, N_CELLS)
    pts = [F.points_of(np.zeros((3, 2))), F.points_of(np.zeros((1, 2)))]
    offs = np.zeros((2, N_ANGLES + 1), np.uint32)
    offs[:, -1] = (3, 1)
    for bad_pts, bad_offs in (([np.zeros(3, np.float32)] * 2, offs), (pts, offs[:1]), (pts, offs.astype(np.int32)), ([], offs), (pts[:1] * 2, offs)):
        with pytest.raises(ValueError):
            o.occupancy_update(bad_pts, bad_offs, g, m)
    for bad_states in (np.zeros((1, 4)), np.zeros((2, 3)), np.zeros((2, 4), complex)):
        with pytest.raises(ValueError):
            o.occupancy_update(pts, offs, g, m, states=bad_states)
    for bad_ev in (np.zeros((8, 9), np.int32), np.zeros((8, 8), np.int64), np.zeros((8, 8), np.uint8)):
        with pytest.raises(ValueError):
            o.occupancy_update(pts, offs, g, m, evidence=bad_ev)
        with pytest.raises(ValueError):
            o.occupancy_map(bad_ev, g)
    for bad_m in ("model", dict(m, l_hit=0), dict(m, margin_bins=N_CELLS + 1), dict(m, max_free_bin=N_CELLS + 1), dict(m, decay=1)):
        with pytest.raises((ValueError, TypeError)):
            o.occupancy_update(pts, offs, g, bad_m)
    with pytest.raises(ValueError):
        o.occupancy_update(pts, offs, "grid", m)
    with pytest.raises(ValueError):
        o.occupancy_update(pts, offs, dict(width=0, height=8, cell=0.5, x0=0.0, y0=0.0), m)
    for n in (0, 65536):
        with pytest.raises(ValueError):
            o.occupancy_update_device(1, 1, n, 4, g, m, 1, 1)
    for mp in (-1, 65537):
        with pytest.raises(ValueError):
            o.occupancy_update_device(1, 1, 2, mp, g, m, 1, 1)
    for args in ((None, 1, 2, 4, g, m, 1, 1), (1, None, 2, 4, g, m, 1, 1), (1, 1, 2, 4, g, m, None, 1), (1, 1, 2, 4, g, m, 1, None)):
        with pytest.raises(ValueError):
            o.occupancy_update_device(*args)
    for args in ((None, g, 1), (1, g, None), (1, "grid", 1)):
        with pytest.raises(ValueError):
            o.occupancy_map_device(*args)
    # max_dist and gate of the grid are not this call's: a config that the field calls refuse passes the grid check
    odd = native.RRFieldConfig(8, 8, 0.5, 0.0, 0.0, 0, -3, 0)
    assert native._grid_cfg(odd).max_dist == 0
    with pytest.raises(ValueError):
        native._field_cfg(odd)
    with pytest.raises(native.RRError, match="rr_set_config"):
        u = _unopened(); u.cfg = None; u.occupancy_update(pts, offs, g, m)


def test_the_facades_have_the_occupancy_call():
    assert callable(radar.RadarHIP.buildOccupancyMap)
    assert "sensor frame into the map frame" in radar.RadarHIP.buildOccupancyMap.__doc__
    hpp = open(os.path.join(ROOT, "include", "radarays_ros_amd", "RadarHIP.hpp")).read()
    for n in ("buildOccupancyMap", "rr_occupancy_config", "rr_field_config"):
        assert n in hpp, n
    marshal = open(os.path.join(ROOT, "include", "radarays_ros_amd", "marshal.hpp")).read()
    assert "rr_occupancy_update" in marshal and "rr_occupancy_map" in marshal


def test_the_cpp_method_compiles():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "occupancy_check.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- kernels ------------------------------------------------------------------------------------------------------------------------------
def test_occupancy_kernels_use_no_scratch(native_lib):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-occupancy"], capture_output=True, text=True, timeout=600)
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
    for k in ("k_occ_profile", "k_occ_free", "k_occ_hit", "k_occ_map"):
        assert k in names, (k, sorted(rows))
    for name, u in rows.items():
        assert u["scratch"] == 0, (name, u)
        assert u["lds"] == 0, (name, u)                                                  # the profile is gathered, nothing is staged
        assert u["vgprs"] <= 64, (name, u)                                               # eight waves per SIMD


def test_occupancy_source_is_in_the_library_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rr_occupancy.hip" in src
    assert re.search(r"^resource-usage-occupancy:", mk, re.M)
    launch = open(os.path.join(CSRC, "rr_launch.h")).read()
    for name in ("occupancy_tile_sizes", "launch_occupancy_update", "launch_occupancy_map"):
        assert len(re.findall(r"\b%s\(" % name, launch)) == 1, name
    images = open(os.path.join(CSRC, "rr_images.hip")).read()
    for n in NEW:
        assert re.search(r"^(int|void) %s\(" % n, images, re.M), n
    assert "k_occ" not in open(os.path.join(CSRC, "rr_field.hip")).read()


# ---- the closed loop, on the oracle's images ----------------------------------------------------------------------------------------------
def loop_clouds():
    from oracle import oracle
    s, cfg = icp_ref.loop_scene(), icp_ref.loop_cfg()
    sc = oracle.Scene(s["verts"], s["faces"], s["face_object_id"], use_bvh=0)
    theta_inc = np.float32(-2 * np.pi / icp_ref.LOOP_ANGLES)
    clouds, offs = [], []
    for pose in O.LOOP_POSES + [icp_ref.LOOP_A, icp_ref.LOOP_B]:
        img = oracle.simulate(sc, mats_tuple(params.kaist_materials()), s["object_materials"], cfg, golden_beams(icp_ref.LOOP_SAMPLES),
                              icp_ref.loop_pose(pose), n_angles=icp_ref.LOOP_ANGLES, want_f32=False)[0]
        p, o = detect_ref.detect_frame(img, theta_min=0.0, theta_inc=theta_inc, resolution=cfg.resolution, **icp_ref.LOOP_DET)
        clouds.append(p)
        offs.append(o)
    return clouds[:-2], np.stack(offs[:-2]), clouds[-2], clouds[-1]


def test_closed_loop_on_the_oracles_images():
    clean, offs, scan_a, scan_b = loop_clouds()
    G, cfg, st, m = O.loop_polar(), F.loop_field_cfg(), O.loop_states(), O.LOOP_MODEL
    assert len(clean) == 8 and m["margin_bins"] >= math.ceil(0.71 * cfg.cell / G.resolution) and m["l_hit"] > m["l_free"]
    dirty, doffs, phantom = O.inject_phantom(clean, offs, G)
    assert sum(len(c) for c in dirty) == sum(len(c) for c in clean) + 1
    ev = O.update(dirty, doffs, cfg, G, m, st)
    occ_map = O.to_map(ev)
    occ_raster = F.rasterize(dirty, cfg, st)
    cell, walls = O.loop_checks(occ_raster, occ_map, clean, phantom, cfg, st)              # statements 1 and 2
    # one hit, and the seven other scans saw through it (the phantom's own scan too where the cell's centre lies in the next azimuth)
    assert ev[cell] in (m["l_hit"] - 7 * m["l_free"], m["l_hit"] - 8 * m["l_free"])
    # 3: the lattice search of §23 on the field of this map, against §23's own argmin (one scan rasterised, recomputed here)
    states, xyz = F.loop_lattice()
    own = F.score(scan_b, states, F.distance_field(F.rasterize([scan_a], cfg, F.loop_map_state()), cfg), cfg)
    assert np.allclose(xyz[int(np.argmin(own["sum_d2"]))], O.LOOP_FIELD_NODE)
    rec = F.score(scan_b, states, F.distance_field(occ_map, cfg, 129), cfg)
    best = int(np.argmin(rec["sum_d2"]))
    order = np.sort(rec["sum_d2"])
    print("closed loop on the oracle's images: phantom cell %s raster %d map %d; %d wall cells, the weakest at %d; %d cells occupied, %d free; "
          "argmin node (%.2f m, %.2f m, %.1f deg) at sum_d2 %d, the next at %d"
          % (cell, occ_raster[cell], occ_map[cell], int(walls.sum()), int(occ_map[walls].min()), int((occ_map > 128).sum()), int((occ_map < 128).sum()),
             xyz[best][0], xyz[best][1], math.degrees(xyz[best][2]), order[0], order[1]))
    O.loop_argmin_check(xyz[best])
    assert order[0] < order[1]                                                             # the argmin is unique
