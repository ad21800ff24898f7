"""Scan matching without a GPU: the flags and tile sizes are as stated (names, prototypes and the layout of rr_icp_rec: tests/test_abi.py), the numpy
restatement (tests/icp_ref.py) gives hand-worked answers, the closed loop's bound is measured on the oracle's images, the Python wrappers
refuse bad arguments before any call into the library, and the kernels of rr_icp.hip use no scratch and the LDS they were designed for."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import detect_ref
import icp_ref as R
from common import golden_beams, mats_tuple
from radarays_ros_amd import native, params, radar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radarays_ros_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "radarays_mi355.h")
STEP = 1.0 / 256.0


def test_icp_entry_points_are_declared_and_exported(native_lib):
    """(names, argument types and struct layouts: tests/test_abi.py, for the whole header)"""
    header = open(HEADER).read()
    assert "#define RR_ABI_VERSION 7" in header
    assert native_lib.lib().rr_abi_version() == 7
    assert re.search(r"#define RR_ICP_DEGENERATE 1u", header) and re.search(r"#define RR_ICP_TRUNCATED 2u", header)
    assert (native_lib.ICP_DEGENERATE, native_lib.ICP_TRUNCATED) == (1, 2)
    src, tgt = native_lib.icp_tile_sizes()
    assert src >= 64 and src % 64 == 0 and tgt >= 2 and tgt % 2 == 0


# ---- the restatement on hand-worked cases -----------------------------------------------------------------------------
def lattice(nx, ny, step=2.0):
    g = np.stack(np.meshgrid(np.arange(nx) * step, np.arange(ny) * step, indexing="ij"), -1).reshape(-1, 2)
    return g.astype(np.float32)


def test_identical_clouds_give_identity():
    cloud = np.random.RandomState(1).uniform(-20, 20, (37, 2)).astype(np.float32)
    recs, states, corr = R.register([cloud], cloud, None, 1.0, 3)
    r = recs[0]
    assert (r["c"], r["s"], r["tx"], r["ty"]) == (1.0, 0.0, 0.0, 0.0)
    assert r["sse"] == 0 and r["n_matched"] == 37 and r["flags"] == 0
    assert np.array_equal(corr[0], np.arange(37)) and np.all(states == [1.0, 0.0, 0.0, 0.0])


def test_a_small_translation_is_recovered_in_one_iteration():
    tgt = lattice(5, 4)                                             # neighbours 2 m apart
    shift = np.array([0.4, -0.3], np.float32)                       # well inside half the spacing: every point finds its own
    recs, _, corr = R.register([tgt - shift], tgt, None, 1.0, 1)
    r = recs[0]
    assert np.array_equal(corr[0], np.arange(len(tgt))) and r["n_matched"] == len(tgt) and r["flags"] == 0
    assert abs(r["tx"] - 0.4) <= STEP and abs(r["ty"] + 0.3) <= STEP and abs(R.yaw_of(r)) <= 1e-3
    assert r["sse"] <= 2 * len(tgt)                                 # a quantisation step per coordinate at the most


def test_a_quarter_turn_of_three_points_is_recovered_from_a_guess_near_it():
    src = np.array([[2.0, 0.0], [5.0, 1.0], [3.0, 4.0]], np.float32)
    tgt = np.stack([-src[:, 1], src[:, 0]], -1) + np.float32([1.0, 2.0])        # turned by +90 degrees, then moved
    init = native.se2_states(math.radians(80.0), 0.8, 1.7)
    recs, _, corr = R.register([src], tgt, init, 3.0, 4)
    r = recs[0]
    assert list(corr[0]) == [0, 1, 2] and r["flags"] == 0
    assert abs(R.yaw_of(r) - math.pi / 2) <= 2e-3 and abs(r["tx"] - 1.0) <= 2 * STEP and abs(r["ty"] - 2.0) <= 2 * STEP


def test_duplicate_target_points_match_the_lower_index():
    tgt = np.array([[9.0, 9.0], [1.0, 1.0], [1.0, 1.0], [5.0, 5.0], [1.0, 1.0]], np.float32)
    _, _, corr = R.register([np.array([[1.1, 0.9], [5.0, 5.2]], np.float32)], tgt, None, 1.0, 0)
    assert list(corr[0]) == [1, 3]


def test_the_gate_is_inclusive():
    gate = np.float32(0.75)
    gate2 = gate * gate
    d = np.float32(np.sqrt(np.float64(gate2)))                      # 0.75 exactly: d * d == gate2
    assert d * d == gate2
    above = np.nextafter(gate2, np.float32(np.inf))
    tgt = np.zeros((1, 2), np.float32)
    recs, _, corr = R.register([np.array([[d, 0.0]], np.float32)], tgt, None, gate, 0)
    assert recs[0]["n_matched"] == 1 and corr[0][0] == 0
    # the next float32 above gate2: 0.75^2 + (2^-12)^2 = 0.5625 + 2^-24, exact in every step
    e = np.float32(2.0 ** -12)
    assert d * d + e * e == above
    recs, _, corr = R.register([np.array([[d, e]], np.float32)], tgt, None, gate, 0)
    assert recs[0]["n_matched"] == 0 and corr[0][0] == R.NONE


def test_too_few_matches_are_degenerate_and_leave_the_state():
    tgt = lattice(3, 3)
    init = native.se2_states(0.3, 0.25, -0.5)
    want = R.normalise(init[0])[0]
    # one point
    recs, states, _ = R.register([tgt[:1]], tgt, init, 1.0, 3)
    assert recs[0]["flags"] == R.DEGENERATE and (recs[0]["c"], recs[0]["s"], recs[0]["tx"], recs[0]["ty"]) == want
    assert np.all(states[:, 0] == want)
    # every point beyond the gate
    recs, _, corr = R.register([tgt + np.float32(100.0)], tgt, init, 1.0, 2)
    assert recs[0]["flags"] == R.DEGENERATE and recs[0]["n_matched"] == 0 and recs[0]["sse"] == 0
    assert (recs[0]["c"], recs[0]["s"], recs[0]["tx"], recs[0]["ty"]) == want and np.all(corr[0] == R.NONE)
    # two coincident pairs: no direction (h == 0)
    recs, _, _ = R.register([np.zeros((2, 2), np.float32)], np.zeros((1, 2), np.float32), None, 1.0, 1)
    assert recs[0]["flags"] == R.DEGENERATE and recs[0]["n_matched"] == 2


def test_nan_sources_and_out_of_range_targets_are_skipped():
    tgt = np.array([[1.0, 1.0], [8192.0, 1.0], [np.nan, 2.0], [3.0, -np.inf], [4.0, 4.0], [-8192.0, 0.0]], np.float32)
    src = np.array([[1.0, 1.1], [np.nan, 1.0], [8191.9, 1.0], [4.0, np.nan], [4.1, 4.0], [9000.0, 1.0]], np.float32)
    recs, _, corr = R.register([src], tgt, None, 2.0, 0)
    assert list(corr[0]) == [0, R.NONE, R.NONE, R.NONE, 4, R.NONE]
    assert recs[0]["n_matched"] == 2 and recs[0]["flags"] == 0
    # with a wide gate the in-range point next to the out-of-range targets takes the nearest VALID one
    _, _, corr = R.register([src[2:3]], tgt, None, 8190.0, 0)
    assert corr[0][0] == 4
    # only invalid targets: nothing is a candidate
    recs, _, corr = R.register([src], tgt[[1, 2, 3, 5]], None, 2.0, 1)
    assert np.all(corr[0] == R.NONE) and recs[0]["flags"] == R.DEGENERATE


def test_zero_iterations_return_the_normalised_initial_state():
    tgt = lattice(3, 3)
    init = np.array([[3.0, 4.0, 0.5, -0.25], [0.0, 0.0, 1.0, 1.0], [np.inf, 1.0, 0.0, 0.0]])
    recs, states, _ = R.register([tgt, tgt, tgt], tgt, init, 1.0, 0)
    assert (recs[0]["c"], recs[0]["s"], recs[0]["tx"], recs[0]["ty"]) == (3.0 / 5.0, 4.0 / 5.0, 0.5, -0.25) and recs[0]["flags"] == 0
    for f in (1, 2):                                                # no direction: the identity, flagged
        assert (recs[f]["c"], recs[f]["s"], recs[f]["tx"], recs[f]["ty"]) == (1.0, 0.0, 0.0, 0.0) and recs[f]["flags"] == R.DEGENERATE
        assert recs[f]["n_matched"] == 9 and recs[f]["sse"] == 0
    assert states.shape == (1, 3, 4)


def test_truncation_is_flagged_and_cuts_the_cloud():
    tgt = lattice(4, 4)
    recs, _, corr = R.register([tgt, tgt[:3]], tgt, None, 1.0, 1, max_points=5)
    assert recs[0]["flags"] == R.TRUNCATED and len(corr[0]) == 5 and recs[1]["flags"] == 0 and len(corr[1]) == 3
    recs, _, corr = R.register([tgt], tgt, None, 1.0, 0, max_tgt=7)
    assert recs[0]["flags"] == R.TRUNCATED and recs[0]["n_matched"] == 7 and np.all(corr[0][7:] == R.NONE)


def test_se2_states_and_the_pose_convention():
    st = native.se2_states([0.0, math.pi / 2], [1.0, 2.0], 3.0)
    assert st.dtype == np.float64 and st.shape == (2, 4) and np.allclose(st, [[1, 0, 1, 3], [0, 1, 2, 3]], atol=1e-15)
    # T = X^-1 X_h: with X the origin, T is the hypothesis' own planar pose, and X_h T^-1 is the origin again
    rec = np.zeros(1, native.ICP_DTYPE)
    rec["c"], rec["s"], rec["tx"], rec["ty"] = math.cos(0.3), math.sin(0.3), 1.5, -0.5
    assert np.allclose(R.compose_inverse((1.5, -0.5, 0.3), rec[0]), (0.0, 0.0, 0.0), atol=1e-12)
    from radarays_ros_amd import scenes
    out = radar.RadarHIP._corrected_by(scenes.yaw_pose(1.5, -0.5, 0.7, 0.3)[None], rec)
    assert np.allclose(out[0], [0, 0, 0, 1, 0, 0, 0.7], atol=1e-6)


# ---- the closed loop's bound, measured here on the oracle's images ---------------------------------------------------------
def loop_clouds():
    from oracle import oracle
    s, cfg = R.loop_scene(), R.loop_cfg()
    sc = oracle.Scene(s["verts"], s["faces"], s["face_object_id"], use_bvh=0)
    theta_inc = np.float32(-2 * np.pi / R.LOOP_ANGLES)
    clouds = []
    for pose in (R.LOOP_A, R.LOOP_B):
        img = oracle.simulate(sc, mats_tuple(params.kaist_materials()), s["object_materials"], cfg, golden_beams(R.LOOP_SAMPLES), R.loop_pose(pose),
                              n_angles=R.LOOP_ANGLES, want_f32=False)[0]
        clouds.append(detect_ref.detect_frame(img, theta_min=0.0, theta_inc=theta_inc, resolution=cfg.resolution, **R.LOOP_DET)[0])
    return clouds


def test_closed_loop_bound_on_the_oracles_images():
    a, b = loop_clouds()
    assert len(a) >= 100 and len(b) >= 100
    recs, _, _ = R.register([b], a, None, R.LOOP_GATE, R.LOOP_ITERATIONS)
    yaw_err, t_err = R.loop_errors(recs[0])
    ident = np.zeros(1, native.ICP_DTYPE)
    ident["c"] = 1.0
    yaw0, t0 = R.loop_errors(ident[0])
    print("closed loop on the oracle's images: yaw error %.4f deg (identity %.4f), translation error %.4f m (identity %.4f), %d of %d matched"
          % (math.degrees(yaw_err), math.degrees(yaw0), t_err, t0, recs[0]["n_matched"], len(b)))
    assert recs[0]["flags"] == 0
    assert yaw_err < yaw0 and t_err < t0                              # the condition: better than the guess in both
    assert yaw_err <= R.LOOP_YAW_BOUND and t_err <= R.LOOP_T_BOUND    # twice the measured value
    # the constants are what is measured here, to the digits given
    assert abs(yaw_err - R.LOOP_YAW_MEASURED) <= math.radians(0.001) and abs(t_err - R.LOOP_T_MEASURED) <= 1e-4


# ---- wrappers refuse before the library -------------------------------------------------------------------------------
def _unopened(n_cells=64, n_angles=16):
    o = native.Context.__new__(native.Context)
    o._h = None
    o._L = None
    o.cfg = params.RadarModelConfig(n_cells=n_cells)
    o.n_angles = n_angles
    return o


def test_wrappers_refuse_bad_arguments_before_the_library():
    o = _unopened()
    pts = [R.points_of(lattice(2, 2)), R.points_of(lattice(1, 2))]
    offs = np.zeros((2, 17), np.uint32)
    offs[:, -1] = (4, 2)
    tgt = R.points_of(lattice(3, 3))
    good_init = native.se2_states([0.0, 0.1])
    for bad_pts, bad_offs, bad_tgt in (([np.zeros(3, np.float32)] * 2, offs, tgt), (pts, offs[:1], tgt), (pts, offs.astype(np.int32), tgt),
                                       (pts[:1] * 2, offs, tgt), ([], offs, tgt), (pts, offs, np.zeros((3, 2), np.float32)),
                                       (pts, offs, tgt.reshape(3, 3)), (pts, offs, np.zeros(65537, native.POINT_DTYPE))):
        with pytest.raises(ValueError):
            o.register_points(bad_pts, bad_offs, bad_tgt)
    for bad_init in (good_init[:1], good_init[:, :3], np.zeros((2, 4)), np.array([[np.nan, 1, 0, 0], [1, 0, 0, 0]]),
                     np.array([[np.inf, 1, 0, 0], [1, 0, 0, 0]]), good_init.astype(complex)):
        with pytest.raises(ValueError):
            o.register_points(pts, offs, tgt, init=bad_init)
    for gate in (0.0, -1.0, float("nan"), float("inf"), 1e39, 1e-50, "wide", True):
        with pytest.raises(ValueError):
            o.register_points(pts, offs, tgt, gate=gate)
        with pytest.raises(ValueError):
            o.register_points_device(1, 1, 2, 4, 1, 1, 9, 1, gate=gate)
    for it in (-1, 65, 2.5, True):
        with pytest.raises(ValueError):
            o.register_points(pts, offs, tgt, iterations=it)
        with pytest.raises(ValueError):
            o.register_points_device(1, 1, 2, 4, 1, 1, 9, 1, iterations=it)
    for n in (0, 65536, -1):
        with pytest.raises(ValueError):
            o.register_points_device(1, 1, n, 4, 1, 1, 9, 1)
    for mp, mt in ((65537, 9), (4, 65537), (-1, 9), (4, -1)):
        with pytest.raises(ValueError):
            o.register_points_device(1, 1, 2, mp, 1, 1, mt, 1)
    for args in ((None, 1, 2, 4, 1, 1, 9, 1), (1, None, 2, 4, 1, 1, 9, 1), (1, 1, 2, 4, None, 1, 9, 1), (1, 1, 2, 4, 1, None, 9, 1),
                 (1, 1, 2, 4, 1, 1, 9, None)):
        with pytest.raises(ValueError):
            o.register_points_device(*args)
    with pytest.raises(native.RRError, match="rr_set_config"):
        u = _unopened(); u.cfg = None; u.register_points(pts, offs, tgt)


def test_the_facades_have_the_registration_call():
    assert callable(radar.RadarHIP.registerPointClouds)
    assert "T = X^-1 X_h" in radar.RadarHIP.registerPointClouds.__doc__
    hpp = open(os.path.join(ROOT, "include", "radarays_ros_amd", "RadarHIP.hpp")).read()
    for n in ("registerPointClouds", "rr_register_points", "rr_icp_rec"):
        assert n in hpp, n


def test_cpp_corrected_pose_equals_the_python_one(native_lib, tmp_path):
    """RadarHIP::correctedPose compiled with g++ against RadarHIP._corrected_by on random tilted poses and records: the two
    restatements of X_h T^-1 must not drift apart"""
    native_lib.build()
    rs = np.random.RandomState(5)
    n = 16
    q = rs.standard_normal((n, 4))
    poses = np.concatenate([q / np.linalg.norm(q, axis=1, keepdims=True), rs.uniform(-20, 20, (n, 3))], 1).astype(np.float32)
    rec = np.zeros(n, native.ICP_DTYPE)
    yaw = rs.uniform(-3, 3, n)
    rec["c"], rec["s"], rec["tx"], rec["ty"] = np.cos(yaw), np.sin(yaw), rs.uniform(-2, 2, n), rs.uniform(-2, 2, n)
    prog = tmp_path / "corrected.cpp"
    prog.write_text("""#include <cstdio>
#include "radarays_ros_amd/RadarHIP.hpp"
int main() {
    float pose[7]; rr_icp_rec r{};
    while (std::scanf("%f %f %f %f %f %f %f %lf %lf %lf %lf", pose, pose + 1, pose + 2, pose + 3, pose + 4, pose + 5, pose + 6, &r.c, &r.s, &r.tx, &r.ty) == 11) {
        const auto o = radarays_ros_amd::RadarHIP::correctedPose(pose, r);
        std::printf("%.9g %.9g %.9g %.9g %.9g %.9g %.9g\\n", o[0], o[1], o[2], o[3], o[4], o[5], o[6]);
    }
    return 0;
}
""")
    exe = tmp_path / "corrected"
    lib_dir = os.path.join(ROOT, "radarays_ros_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe), "-L", lib_dir, "-lradarays_mi355",
                    "-Wl,-rpath," + lib_dir], check=True)
    lines = "".join(" ".join(repr(float(v)) for v in list(poses[k]) + [rec["c"][k], rec["s"][k], rec["tx"][k], rec["ty"][k]]) + "\n" for k in range(n))
    out = subprocess.run([str(exe)], input=lines, check=True, capture_output=True, text=True).stdout
    got = np.array([[float(v) for v in ln.split()] for ln in out.splitlines()], np.float32)
    want = radar.RadarHIP._corrected_by(poses, rec)
    assert got.shape == want.shape == (n, 7)
    # both compute in f64 from the same f32 pose and round once to f32: equal up to the last bit of libm's sin / cos / atan2
    assert np.allclose(got, want, rtol=0, atol=4e-6), np.abs(got - want).max()
    assert np.abs(want - poses).max() > 0.5                           # the correction is not a no-op


# ---- kernels ----------------------------------------------------------------------------------------------------------
def test_icp_kernels_use_no_scratch_and_the_lds_they_were_designed_for(native_lib):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-icp"], capture_output=True, text=True, timeout=600)
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
    for k in ("k_icp_init", "k_icp_pass", "k_icp_solve"):
        assert k in names, (k, sorted(rows))
    _, tgt_tile = native_lib.icp_tile_sizes()
    for name, u in rows.items():
        assert u["scratch"] == 0, (name, u)
        assert u["lds"] == (8 * tgt_tile if "k_icp_pass" in name else 0), (name, u)      # one (x, y) f32 pair per target of a tile
        assert u["vgprs"] <= 128, (name, u)                                             # four waves per SIMD at the least


def test_icp_source_is_in_the_library_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rr_icp.hip" in src
    assert re.search(r"^resource-usage-icp:", mk, re.M)
