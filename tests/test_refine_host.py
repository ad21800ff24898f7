"""Map refinement without a GPU: the two-pass construction of the nearest-cell transform equals the definition (the minimum 64-bit key over the
list of occupied cells) on every grid, map and saturation of the GPU tests, and keeps the invariant against the distance field; the numpy
restatement (tests/refine_ref.py) gives hand-worked answers; the ABI version has not moved and the new symbols are exported; the wrappers
refuse bad arguments before any call into the library; the façades have the methods and the C++ one compiles; the kernels of rr_refine.hip use
no scratch memory; and the closed loop's figures are measured on the oracle's images."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import field_ref as F
import icp_ref
import refine_ref as R
from radarays_ros_amd import native, params, radar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radarays_ros_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "radarays_mi355.h")
NEW = ["rr_nearest_field_device", "rr_nearest_field", "rr_refine_poses_device", "rr_refine_poses", "rr_refine_tile_sizes"]


# ---- the transform: the construction against the definition, and the invariant against the distance field -----------------------------
def _grids():
    return R.grid_list(native.refine_tile_sizes()[2])


@pytest.mark.parametrize("case", range(12))
def test_the_two_pass_construction_is_the_minimum_key(case):
    W, H = _grids()[case]
    for name, occ in R.map_list(W, H).items():
        for md in R.MAX_DISTS:
            cfg = R.grid_cfg(W, H, md)
            got = R.nearest_field(occ, cfg)
            assert got.dtype == np.uint32 and got.shape == (H, W)
            assert np.array_equal(got, R.nearest_field_brute(occ, cfg)), (W, H, name, md)
            fld = F.distance_field(occ, cfg).astype(np.int64)
            some, d2 = R.nearest_d2(got, cfg)
            assert np.array_equal(some, fld < md * md), (W, H, name, md)          # NONE iff cap2 ...
            assert np.array_equal(d2[some], fld[some]), (W, H, name, md)          # ... else the field's own value
            assert np.all(occ.reshape(-1)[got[some]] == 1)                        # and what it names is occupied
            if not occ.any():
                assert np.all(got == R.NONE)


def test_ties_go_to_the_lowest_linear_index():
    occ = np.zeros((5, 5), np.uint8)
    occ[0, 2] = occ[2, 0] = occ[2, 4] = occ[4, 2] = 1                 # four cells at distance 2 from the centre
    cfg = R.grid_cfg(5, 5, 4)
    got = R.nearest_field(occ, cfg)
    assert got[2, 2] == 0 * 5 + 2                                     # the lowest row wins
    assert got[2, 1] == 2 * 5 + 0 and got[2, 3] == 2 * 5 + 4 and got[1, 1] == 0 * 5 + 2 and got[3, 1] == 2 * 5 + 0
    col = np.zeros((5, 1), np.uint8)
    col[0, 0] = col[4, 0] = 1
    assert list(R.nearest_field(col, R.grid_cfg(1, 5, 4)).ravel()) == [0, 0, 0, 4, 4]     # above and below tie at iy = 2: the lower jy
    lone = np.zeros((3, 9), np.uint8)
    lone[1, 0] = 1
    got = R.nearest_field(lone, R.grid_cfg(9, 3, 3))
    assert list(got[1]) == [9, 9, 9] + [R.NONE] * 6 and got[0, 2] == 9 and got[0, 3] == R.NONE          # d2 < cap2 = 9 only
    assert np.array_equal(R.nearest_field(np.array([[5, 200]], np.uint8), R.grid_cfg(2, 1, 2), threshold=129), np.array([[1, 1]], np.uint32))


# ---- the restatement of the refinement on hand-worked cases ------------------------------------------------------------------------------
def _wall_map():
    """an L of occupied cells on a 24 x 20 grid of 0.5 m cells from (-6, -5)"""
    cfg = native.field_config(24, 20, 0.5, -6.0, -5.0, 6, 3)
    occ = np.zeros((20, 24), np.uint8)
    occ[3, 2:22] = 1
    occ[3:18, 21] = 1
    return cfg, occ


def test_cell_centres_at_the_identity_cost_nothing():
    cfg, occ = _wall_map()
    near = R.nearest_field(occ, cfg)
    index = np.nonzero(occ.reshape(-1))[0]
    scan = R.cell_centres(index, cfg)
    for it in (0, 3):
        rec = R.refine(scan, native.se2_states(0.0), near, cfg, it)[0]
        assert rec["sse"] == 0 and rec["n_matched"] == len(scan) and rec["flags"] == 0
        assert (rec["c"], rec["s"]) == (1.0, 0.0) and abs(rec["tx"]) < 1e-12 and abs(rec["ty"]) < 1e-12
    # ... and a small offset is pulled back onto them: every point returns to its own cell's centre
    moved = R.refine(scan, native.se2_states(0.0, 0.11, -0.07), near, cfg, 2)[0]
    # (to within half a quantisation step of 1/256 m: the solve sees the offset as 28/256 and -18/256)
    assert moved["sse"] == 0 and moved["n_matched"] == len(scan) and abs(moved["tx"]) <= 1 / 512 and abs(moved["ty"]) <= 1 / 512
    assert abs(moved["tx"] - (0.11 - 28 / 256)) < 1e-12 and abs(moved["ty"] - (-0.07 + 18 / 256)) < 1e-12
    still = R.refine(scan, native.se2_states(0.0, 0.11, -0.07), near, cfg, 0)[0]
    assert still["sse"] == len(scan) * (round(0.11 * 256) ** 2 + round(0.07 * 256) ** 2) and (still["tx"], still["ty"]) == (0.11, -0.07)


def test_degenerate_truncated_and_nan_states():
    cfg, occ = _wall_map()
    near = R.nearest_field(occ, cfg)
    scan = R.cell_centres(np.nonzero(occ.reshape(-1))[0], cfg)
    init = np.array([[0.0, 0.0, 1.0, 1.0], [np.nan, 0.0, 0.0, 0.0], [1.0, 0.0, np.nan, 0.0], [1.0, 0.0, 500.0, 0.0], [3.0, 4.0, 0.0, 0.0]])
    rec = R.refine(scan, init, near, cfg, 2)
    for h in (0, 1):                                                  # no direction: the identity, flagged, and then refined like it
        assert rec[h]["flags"] == R.DEGENERATE and (rec[h]["c"], rec[h]["s"]) == (1.0, 0.0) and rec[h]["sse"] == 0
    assert rec[2]["flags"] == R.DEGENERATE and rec[2]["n_matched"] == 0 and np.isnan(rec[2]["tx"]) and rec[2]["c"] == 1.0
    assert rec[3]["flags"] == R.DEGENERATE and rec[3]["n_matched"] == 0 and (rec[3]["tx"], rec[3]["ty"]) == (500.0, 0.0)   # off the grid: unchanged
    assert rec[4]["flags"] == 0 and abs(math.hypot(rec[4]["c"], rec[4]["s"]) - 1.0) < 1e-15
    zero = R.refine(scan, init[2:4], near, cfg, 0)                    # no solve runs: no flag
    assert list(zero["flags"]) == [0, 0] and list(zero["n_matched"]) == [0, 0]
    cut = R.refine(scan, init[4:], near, cfg, 1, max_points=5)[0]
    assert cut["flags"] == R.TRUNCATED and cut["n_matched"] <= 5
    one = R.refine(scan[:1], native.se2_states(0.0), near, cfg, 1)[0]
    assert one["flags"] == R.DEGENERATE and one["n_matched"] == 1     # fewer than two pairs
    gate0 = native.field_config(24, 20, 0.5, -6.0, -5.0, 6, 0)
    shifted = R.refine(scan, native.se2_states(0.0, 0.6, 0.0), near, gate0, 0)[0]
    assert 0 < shifted["n_matched"] < len(scan)                       # gate 0: only points that fall into an occupied cell


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------------
def test_refine_entry_points_are_declared_and_exported(native_lib):
    """(names, argument types and struct layouts: tests/test_abi.py, for the whole header)"""
    header = open(HEADER).read()
    assert "#define RR_ABI_VERSION 7" in header
    L = native_lib.lib()
    assert L.rr_abi_version() == 7
    for n in NEW:
        assert n in native.SYMBOLS and hasattr(L, n) and re.search(r"\b%s\(" % n, header), n
    points_tile, hyps, row_tile = native_lib.refine_tile_sizes()
    assert points_tile == 64 and hyps >= 1 and row_tile >= 1
    assert native.NEAREST_NONE == 0xFFFFFFFF and native.ICP_DTYPE.itemsize == 48


# ---- wrappers refuse before the library -------------------------------------------------------------------------------------------------
def _unopened():
    o = native.Context.__new__(native.Context)
    o._h = None
    o._L = None
    o.cfg = params.RadarModelConfig(n_cells=64)
    o.n_angles = 16
    return o


def test_wrappers_refuse_bad_arguments_before_the_library():
    o = _unopened()
    g = native.field_config(8, 8, 0.5, 0.0, 0.0, 4, 1)
    for occ in (np.zeros((8, 8), np.uint16), np.zeros((7, 8), np.uint8)):
        with pytest.raises(ValueError):
            o.nearest_field(occ, g)
    for th in (0, 256, 1.5, True):
        with pytest.raises(ValueError):
            o.nearest_field(np.zeros((8, 8), np.uint8), g, threshold=th)
        with pytest.raises(ValueError):
            o.nearest_field_device(1, g, 2, threshold=th)
    for args in ((None, g, 2), (1, g, None), (1, g, 1), (1, "grid", 2)):
        with pytest.raises(ValueError):
            o.nearest_field_device(*args)
    pts, near, st = F.points_of(np.zeros((3, 2))), np.zeros((8, 8), np.uint32), np.zeros((2, 4))
    for bad in ((pts, st[:0], near), (pts, np.zeros((2, 3)), near), (pts, np.zeros((2, 4), complex), near), (pts, st, near.astype(np.uint16)),
                (np.zeros((3, 2)), st, near), (pts, st, np.zeros((8, 7), np.uint32))):
        with pytest.raises(ValueError):
            o.refine_poses(*bad, g)
    for it in (-1, 65, 1.5, True):
        with pytest.raises(ValueError):
            o.refine_poses(pts, st, near, g, iterations=it)
        with pytest.raises(ValueError):
            o.refine_poses_device(1, 1, 4, 1, 2, 1, g, 1, iterations=it)
    for n_hyp in (0, (1 << 22) + 1, -1):
        with pytest.raises(ValueError):
            o.refine_poses_device(1, 1, 4, 1, n_hyp, 1, g, 1)
    for mp in (-1, 65537):
        with pytest.raises(ValueError):
            o.refine_poses_device(1, 1, mp, 1, 2, 1, g, 1)
    for args in ((None, 1, 4, 1, 2, 1, g, 1), (1, None, 4, 1, 2, 1, g, 1), (1, 1, 4, None, 2, 1, g, 1), (1, 1, 4, 1, 2, None, g, 1),
                 (1, 1, 4, 1, 2, 1, g, None)):
        with pytest.raises(ValueError):
            o.refine_poses_device(*args)
    # the 8192 m rule: every extent, taken in f64 from the f32 fields, strictly within +-8192
    for far in (native.field_config(8, 8, 0.5, 8192.0, 0.0, 4, 1), native.field_config(8, 8, 0.5, 0.0, -8192.0, 4, 1),
                native.field_config(8, 8, 0.5, 8188.0, 0.0, 4, 1), native.field_config(8, 8, 0.5, 0.0, 8188.0, 4, 1),
                native.field_config(4096, 8, 4.0, -8192.5, 0.0, 4, 1), native.field_config(4096, 4096, 2.0, -100.0, 0.5, 4, 1)):
        with pytest.raises(ValueError, match="8192"):
            o.refine_poses_device(1, 1, 4, 1, 2, 1, far, 1)
        with pytest.raises(ValueError, match="8192"):
            o.refine_poses(pts, st, np.zeros((far.height, far.width), np.uint32), far)
    native._refine_cfg(native.field_config(8, 8, 0.5, 8187.5, -8191.5, 4, 1))       # 8191.5 and -8187.5: inside
    native._refine_cfg(native.field_config(4096, 4096, 2.0, -4096.0, -4096.0, 4, 1))


def test_the_facades_have_the_refinement_calls():
    assert callable(radar.RadarHIP.buildNearestField) and callable(radar.RadarHIP.refinePoses) and callable(radar.RadarHIP.refineRecords)
    assert "sensor frame into the map frame" in radar.RadarHIP.refinePoses.__doc__
    hpp = open(os.path.join(ROOT, "include", "radarays_ros_amd", "RadarHIP.hpp")).read()
    for n in ("buildNearestField", "refinePoses", "rr_icp_rec", "marshal::refine_poses", "marshal::build_nearest"):
        assert n in hpp, n
    marshal = open(os.path.join(ROOT, "include", "radarays_ros_amd", "marshal.hpp")).read()
    assert "rr_refine_poses_device" in marshal and "rr_nearest_field" in marshal


def test_the_cpp_methods_compile():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "refine_check.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- kernels ------------------------------------------------------------------------------------------------------------------------------
def test_refine_kernels_use_no_scratch(native_lib):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-refine"], capture_output=True, text=True, timeout=600)
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
    for k in ("k_near_columns", "k_near_rows", "k_refine"):
        assert k in names, (k, sorted(rows))
    for name, u in rows.items():
        assert u["scratch"] == 0, (name, u)
        # the staged row of the row pass: 4096 offsets between two aprons of 255, 16 bits each; nothing anywhere else
        assert u["lds"] == (2 * (4096 + 2 * 255) if "k_near_rows" in name else 0), (name, u)
        assert u["vgprs"] <= 256, (name, u)


def test_refine_source_is_in_the_library_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rr_refine.hip" in src
    assert re.search(r"^resource-usage-refine:", mk, re.M)
    launch = open(os.path.join(CSRC, "rr_launch.h")).read()
    for name in ("refine_tile_sizes", "launch_nearest_field", "launch_refine"):
        assert len(re.findall(r"\b%s\(" % name, launch)) == 1, name
    images = open(os.path.join(CSRC, "rr_images.hip")).read()
    for n in NEW:
        assert re.search(r"^(int|void) %s\(" % n, images, re.M), n
    kernels = open(os.path.join(CSRC, "rr_refine.hip")).read()
    assert "atomic" not in kernels.split("namespace rr {", 1)[1] and kernels.count("__syncthreads()") == 1      # the row pass's one barrier


# ---- the closed loop's figures, measured here on the oracle's images ------------------------------------------------------------------------
def test_closed_loop_figure_on_the_oracles_images():
    import filter_ref
    from test_field_host import loop_clouds
    a, b = loop_clouds()
    assert len(a) >= 100 and len(b) >= 100
    cfg = R.loop_field_cfg()
    occ = F.rasterize([a], cfg, F.loop_map_state())
    near = R.nearest_field(occ, cfg)
    assert np.array_equal(near, R.nearest_field_brute(occ, cfg))
    rec = R.refine(b, R.loop_guess(), near, cfg, R.LOOP_ITERATIONS)[0]
    eyaw, et = R.loop_errors(rec)
    print("closed loop on the oracle's images: from A's own state (%.3f deg, %.4f m off) %d iterations at gate %d end %.4f deg and %.4f m off "
          "the truth, sse %d over %d pairs" % (math.degrees(R.LOOP_GUESS_YAW), R.LOOP_GUESS_T, R.LOOP_ITERATIONS, R.LOOP_GATE, math.degrees(eyaw),
                                             et, rec["sse"], rec["n_matched"]))
    assert rec["flags"] == 0 and rec["n_matched"] == len(b)
    assert eyaw < R.LOOP_GUESS_YAW and et < R.LOOP_GUESS_T            # the result beats the guess in both
    assert eyaw <= R.LOOP_YAW_BOUND and et <= R.LOOP_T_BOUND
    # the constants are what is measured here
    assert abs(eyaw - R.LOOP_YAW_MEASURED) <= math.radians(5e-4) and abs(et - R.LOOP_T_MEASURED) <= 5e-5

    # reported, not asserted: the same refinement from the lattice's argmin node and from the particle filter's best particle
    fld = F.distance_field(occ, cfg)
    states, xyz = F.loop_lattice()
    node = int(np.argmin(F.score(b, states, fld, F.loop_field_cfg())["sum_d2"]))
    fc = native.filter_config(filter_ref.LOOP_SIGMA_XY, filter_ref.LOOP_SIGMA_YAW, filter_ref.LOOP_QUANTUM, filter_ref.LOOP_N_TABLE)
    table = native.filter_weight_table(filter_ref.LOOP_SIGMA_CELLS, filter_ref.LOOP_QUANTUM, filter_ref.LOOP_N_TABLE)
    st = filter_ref.loop_particles()
    for k in range(filter_ref.LOOP_STEPS):
        st = filter_ref.step(lambda x: F.score(b, x, fld, F.loop_field_cfg()), st, table, filter_ref.LOOP_QUANTUM, filter_ref.loop_phase(k),
                             (1, 0, 0, 0), fc.sigma_xy, fc.sigma_t, filter_ref.LOOP_SEED, k)[4]
    best = int(np.argmin(F.score(b, st, fld, F.loop_field_cfg())["sum_d2"]))
    for name, start in (("the lattice's argmin node", states[node]), ("the filter's best particle", st[best])):
        before = np.zeros(1, native.ICP_DTYPE)
        before["c"], before["s"], before["tx"], before["ty"] = (float(v) for v in start)
        y0, t0 = R.loop_errors(before[0])
        y1, t1 = R.loop_errors(R.refine(b, np.asarray(start, np.float64)[None], near, cfg, R.LOOP_ITERATIONS)[0])
        print("  from %s (%.3f deg, %.4f m off): %.4f deg, %.4f m off" % (name, math.degrees(y0), t0, math.degrees(y1), t1))
