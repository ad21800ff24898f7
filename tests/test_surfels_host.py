"""Oriented surface points and point-to-line scan matching without a GPU: the entry points and records are as stated (names, prototypes and
layouts: tests/test_abi.py), every refusal code, the numpy restatement (tests/surfels_ref.py) on hand-worked cases, a fixed point on two
perpendicular walls, the closed loop of DESIGN.md §22's room on the oracle's images, in which point-to-line must beat point-to-point, and
the kernels of rr_surfels.hip use no scratch and the LDS they were designed for."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import icp_ref as P
import detect_ref
import surfels_ref as R
from common import golden_beams, mats_tuple
from radarays_ros_amd import native, params, radar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radarays_ros_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "radarays_mi355.h")
NEW = ["rr_surfels_scratch_bytes", "rr_surfels_tile_sizes", "rr_surface_points_device", "rr_surface_points", "rr_register_surfels_device",
       "rr_register_surfels"]


def test_entry_points_are_exported_and_the_abi_is_still_7(native_lib):
    header = open(HEADER).read()
    assert "#define RR_ABI_VERSION 7" in header and native_lib.lib().rr_abi_version() == 7
    for n in NEW:
        assert hasattr(native_lib.lib(), n) and n in native_lib.PROTOTYPES, n
    assert re.search(r"#define RR_SURFELS_TRUNCATED 1u", header) and re.search(r"#define RR_SURFELS_CAPPED\s+2u", header)
    assert (native_lib.SURFELS_TRUNCATED, native_lib.SURFELS_CAPPED) == (1, 2)
    assert C.sizeof(native_lib.RRSurfel) == native_lib.SURFEL_DTYPE.itemsize == 32 and C.sizeof(native_lib.RRSurfelConfig) == 32
    assert C.sizeof(native_lib.RRIcpRec) == 48                        # the record is rr_register_points' own
    points_tile, chunk = native_lib.surfels_tile_sizes()
    assert points_tile % 64 == 0 and chunk % points_tile == 0


def test_scratch_bytes_and_the_refusals_that_need_no_context(native_lib):
    """the shape check behind rr_surfels_scratch_bytes and the -1 of every entry point; -2 and -3 need a context, which needs a device:
    tests/test_gpu_surfels.py holds them (test_surface_points_refusals, test_register_refusals)"""
    L = native_lib.lib()
    g = native_lib.surfel_config(1.0, 8)
    need = L.rr_surfels_scratch_bytes(3, C.byref(g))
    assert need >= 3 * 64 * 48 + 3 * 64 and need % 16 == 0
    assert L.rr_surfels_scratch_bytes(0, C.byref(g)) == 0 and L.rr_surfels_scratch_bytes(65536, C.byref(g)) == 0 and L.rr_surfels_scratch_bytes(1, None) == 0
    for field, v in (("cell", 0.0), ("cell", 16.01), ("cell", 0.001), ("cell", float("inf")), ("width", 0), ("width", 1025), ("min_points", 1),
                     ("min_points", 65537), ("max_ratio", -0.5), ("max_ratio", 1.01), ("max_ratio", float("nan"))):
        bad = native_lib.surfel_config(1.0, 8)
        setattr(bad, field, v)
        assert L.rr_surfels_scratch_bytes(1, C.byref(bad)) == 0, (field, v)
    for ok in (native_lib.surfel_config(1.0 / 256.0, 1024, 2, 0.0), native_lib.surfel_config(16.0, 1, 65536, 1.0)):
        assert L.rr_surfels_scratch_bytes(1, C.byref(ok)) > 0
    p = 4096
    assert L.rr_surface_points_device(None, p, p, 1, 4, C.byref(g), p, 4, p, p, need, None) == -1
    assert L.rr_surface_points(None, p, p, 1, 4, C.byref(g), p, 4, p) == -1
    assert L.rr_register_surfels_device(None, p, p, 1, 4, p, p, 4, None, 1.0, 1, p, None, None) == -1
    assert L.rr_register_surfels(None, p, p, 1, 4, p, 4, 4, None, 1.0, 1, p, None) == -1


def _unopened(n_cells=64, n_angles=16):
    o = native.Context.__new__(native.Context)
    o._h = None
    o._L = None
    o.cfg = params.RadarModelConfig(n_cells=n_cells)
    o.n_angles = n_angles
    return o


def test_wrappers_refuse_bad_arguments_before_the_library():
    o = _unopened()
    for kw in (dict(cell=0.0), dict(cell=17.0), dict(cell="wide"), dict(cell=True), dict(cell=float("nan")), dict(width=0), dict(width=1025),
               dict(width=2.5), dict(min_points=1), dict(min_points=65537), dict(max_ratio=-0.1), dict(max_ratio=1.1), dict(max_ratio="x")):
        with pytest.raises(ValueError):
            native.surfel_config(**dict(dict(cell=1.0, width=8), **kw))
    g = native.surfel_config(1.0, 8)
    bad = native.surfel_config(1.0, 8)
    bad.reserved_[1] = 3
    pts = [P.points_of(np.zeros((4, 2), np.float32))]
    offs = np.zeros((1, 17), np.uint32)
    offs[0, -1] = 4
    for cfg in (bad, None, (1.0, 8), dict(cell=1.0)):
        with pytest.raises((ValueError, TypeError)):
            o.surface_points(pts, offs, cfg)
    for ms in (-1, (1 << 20) + 1, 2.5, True):
        with pytest.raises(ValueError):
            o.surface_points(pts, offs, g, ms)
    with pytest.raises(ValueError):
        o.surface_points(pts, offs[:, :5], g)
    good = (16, 16, 1, 4, g, 16, 4, 16, 16, 1 << 30)
    for at, v in ((0, None), (1, None), (2, 0), (2, 65536), (3, 65537), (3, -1), (5, None), (5, 24), (6, 0), (6, -1), (7, None), (7, 18), (8, None),
                  (8, 24), (9, 0), (9, True), (9, 2.5)):
        a = list(good)
        a[at] = v
        with pytest.raises(ValueError):
            o.surface_points_device(*a)
    tgt = np.zeros(3, native.SURFEL_DTYPE)
    for bad_tgt in (np.zeros(3, native.POINT_DTYPE), tgt.reshape(3, 1), np.zeros(65537, native.SURFEL_DTYPE)):
        with pytest.raises(ValueError):
            o.register_surfels(pts, offs, bad_tgt)
    for kw in (dict(gate=0.0), dict(gate=float("nan")), dict(iterations=65), dict(iterations=-1), dict(init=np.zeros((1, 4)))):
        with pytest.raises(ValueError):
            o.register_surfels(pts, offs, tgt, **kw)
    for args, kw in (((None, 1, 2, 4, 16, 1, 9, 1), {}), ((1, None, 2, 4, 16, 1, 9, 1), {}), ((1, 1, 2, 4, None, 1, 9, 1), {}), ((1, 1, 2, 4, 16, None, 9, 1), {}),
                     ((1, 1, 2, 4, 16, 1, 9, None), {}), ((1, 1, 0, 4, 16, 1, 9, 1), {}), ((1, 1, 2, 65537, 16, 1, 9, 1), {}), ((1, 1, 2, 4, 16, 1, 65537, 1), {}),
                     ((1, 1, 2, 4, 24, 1, 9, 1), {}), ((1, 1, 2, 4, 16, 1, 9, 1), dict(gate=-1.0)), ((1, 1, 2, 4, 16, 1, 9, 1), dict(iterations=65))):
        with pytest.raises(ValueError):
            o.register_surfels_device(*args, **kw)
    with pytest.raises(native.RRError, match="rr_set_config"):
        u = _unopened(); u.cfg = None; u.surface_points(pts, offs, g)


# ---- the restatement's own properties -----------------------------------------------------------------------------------------------------
def test_collinear_points_have_no_variance_across_and_the_lines_exact_normal():
    xs = np.linspace(-0.9, 0.9, 7, dtype=np.float32)
    for pts, normal in ((np.stack([xs, np.full_like(xs, 2.5)], -1), (0.0, -1.0)),                   # a wall ahead in y: the normal looks back at the origin
                        (np.stack([np.full_like(xs, -2.5), xs], -1), (1.0, 0.0)),
                        (np.stack([xs + 3.0, 3.0 - xs], -1), (-math.sqrt(0.5), -math.sqrt(0.5)))):   # x + y = 6
        s, counts = R.surface_points([pts], 2.0, 8, 3, 0.0)
        assert counts[0, 0] == len(s[0]) >= 1
        for r in s[0]:
            assert r["var_n"] == 0.0 and r["var_t"] > 0.0
            assert (r["nx"], r["ny"]) == (np.float32(normal[0]), np.float32(normal[1]))
            assert r["nx"] * r["x"] + r["ny"] * r["y"] < 0              # the normal faces the origin


def test_the_normal_faces_the_origin_from_every_side():
    rs = np.random.RandomState(2)
    for ang in np.linspace(0.1, 6.2, 12):
        c, s_ = math.cos(ang), math.sin(ang)
        t = np.linspace(-1.5, 1.5, 25)
        pts = np.stack([5 * c - s_ * t, 5 * s_ + c * t], -1) + rs.normal(0, 0.01, (25, 2))          # a wall 5 m out, square to the line of sight
        s, _ = R.surface_points([pts.astype(np.float32)], 1.0, 16, 3, 0.1)
        assert len(s[0]) >= 2
        for r in s[0]:
            assert r["nx"] * r["x"] + r["ny"] * r["y"] < 0 and abs(math.hypot(r["nx"], r["ny"]) - 1) < 1e-6
            assert abs(r["nx"] + c) < 0.05 and abs(r["ny"] + s_) < 0.05 and r["var_n"] < 1e-3 < r["var_t"]


def test_floor_rule_repeated_point_symmetric_square_and_the_cap():
    sums = R.cell_sums(np.array([[-1.0, -1.0], [-1.0 / 256, -1.0 / 256], [0.0, 0.0]], np.float32), 256, 8)
    assert sorted(sums) == [27, 36]                                    # -1 m and -1/256 m floor to cell (3, 3); truncation would put the latter in (4, 4)
    assert sums[27] == [2, 255, 255, 255 * 255, 255 * 255, 255 * 255] and sums[36] == [1, 0, 0, 0, 0, 0]
    one = np.repeat(np.array([[0.3, 0.4]], np.float32), 6, 0)
    square = np.array([[0.25, 0.25], [0.75, 0.25], [0.25, 0.75], [0.75, 0.75]], np.float32)
    s, counts = R.surface_points([one, square], 1.0, 8, 2, 1.0)
    assert counts[:, 0].tolist() == [0, 0]                            # h == 0 both times
    xs = np.linspace(-3.9, 3.9, 60, dtype=np.float32)
    s, counts = R.surface_points([np.stack([xs, np.full_like(xs, 1.5)], -1)], 1.0, 8, 3, 0.1, max_surfels=3)
    assert counts[0].tolist() == [8, R.SF_CAPPED] and len(s[0]) == 3 and np.all(np.diff(s[0]["cell"].astype(int)) > 0)


def two_walls(phase, step):
    xs = np.arange(-6.0 + phase, 6.0, step)
    ys = np.arange(-4.0 + phase, 5.0, step)
    return np.concatenate([np.stack([xs, np.full_like(xs, 5.0)], -1), np.stack([np.full_like(ys, 6.0), ys], -1)])


# measured here (the test prints it): from the identity the restatement ends 0.0063 degrees and 0.0043 m from the truth
FIXED_YAW_MEASURED, FIXED_T_MEASURED = math.radians(0.0063), 0.0043


def test_fixed_point_on_two_perpendicular_walls():
    truth = (0.45, 0.2, math.radians(2.0))
    T = native.se2_states(truth[2], truth[0], truth[1])
    surf, _ = R.surface_points([two_walls(0.0, 0.1).astype(np.float32)], 1.0, 32, 3, 0.1)
    q = two_walls(0.05, 0.13)                                         # another phase and spacing than the target's samples
    c, s, tx, ty = T[0]
    d = q - [tx, ty]
    src = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], -1).astype(np.float32)       # T moves it onto the walls
    recs, states, _ = R.register([src], surf[0], T, 1.0, 10)
    yaw_err, t_err = R.errors(recs[0], truth)
    assert recs[0]["flags"] == 0 and yaw_err <= math.radians(1e-3) and t_err <= 1.0 / 64                  # it stays at the truth, to the quantum
    recs, _, _ = R.register([src], surf[0], None, 1.0, 10)
    yaw_err, t_err = R.errors(recs[0], truth)
    print("fixed point from the identity: yaw error %.5f deg, translation error %.5f m, %d of %d matched" % (math.degrees(yaw_err), t_err, recs[0]["n_matched"], len(src)))
    assert recs[0]["flags"] == 0 and yaw_err <= 2 * FIXED_YAW_MEASURED and t_err <= 2 * FIXED_T_MEASURED  # twice the measured value


def test_degenerate_cases_of_the_restatement():
    xs = np.linspace(-5, 5, 40).astype(np.float32)
    corridor = R.surfels_of(np.stack([xs, np.full_like(xs, 2.0)], -1), np.tile(np.float32([0, -1]), (40, 1)))
    src = np.stack([xs + 0.1, np.full_like(xs, 1.8)], -1)
    recs, states, _ = R.register([src], corridor, None, 1.0, 3)
    assert recs[0]["flags"] == R.DEGENERATE and recs[0]["n_matched"] == 40 and np.all(states == [1.0, 0.0, 0.0, 0.0])
    assert recs[0]["sse"] == 40 * (round(0.2 * 64) * 1024) ** 2       # r = M . e in 1/64 m times 1/1024
    recs, _, corr = R.register([src + np.float32(100)], corridor, None, 1.0, 2)
    assert recs[0]["flags"] == R.DEGENERATE and recs[0]["n_matched"] == 0 and np.all(corr[0] == R.NONE)
    bad = corridor.copy()
    bad["nx"][::2], bad["y"][1::4] = 1.5, np.nan
    _, _, corr = R.register([src], bad, None, 3.0, 0)
    assert np.all(corr[0] % 4 == 3)                                   # only the surfels left untouched are candidates


def test_a_corridor_in_a_general_direction_is_flagged_but_may_slide_first():
    """the stated limit, pinned: with all normals parallel H is exactly singular, but for a direction that is neither an axis nor a diagonal
    the f64 pivots carry rounding, so a solve may see a tiny positive d2 and move the state ALONG the wall before a later solve sees a pivot
    that is not > 0 and flags the frame.  Within three iterations every such frame is flagged; its state is not guaranteed to be kept"""
    moved = 0
    for angle in R.GENERAL_CORRIDORS:
        tgt, src = R.corridor(angle)
        recs, states, _ = R.register([src], tgt, None, 1.5, 3)
        assert recs[0]["flags"] == R.DEGENERATE and recs[0]["n_matched"] == 40, angle
        n = (math.cos(angle), math.sin(angle))
        along = -float(recs[0]["tx"]) * n[1] + float(recs[0]["ty"]) * n[0]
        print("corridor at %.4f rad: state (%.6f, %.6f, %.4f, %.4f), slid %.4f m along the wall" % (angle, recs[0]["c"], recs[0]["s"], recs[0]["tx"], recs[0]["ty"], along))
        moved += bool(np.any(states[-1, 0] != [1.0, 0.0, 0.0, 0.0]))
        assert abs(along) <= 0.5 and abs(math.atan2(recs[0]["s"], recs[0]["c"])) <= 1e-3      # what was measured here: 0.18 m at the most, no turn
    assert moved >= 1                                                  # the limit is real: at least one of them slid before it was flagged


# ---- the closed loop of DESIGN.md §22 on the oracle's images ----------------------------------------------------------------------------
def loop_clouds():
    """the two clouds of test_icp_host.py's closed loop, from the oracle's images"""
    from oracle import oracle
    s, cfg = P.loop_scene(), P.loop_cfg()
    sc = oracle.Scene(s["verts"], s["faces"], s["face_object_id"], use_bvh=0)
    theta_inc = np.float32(-2 * np.pi / P.LOOP_ANGLES)
    clouds = []
    for pose in (P.LOOP_A, P.LOOP_B):
        img = oracle.simulate(sc, mats_tuple(params.kaist_materials()), s["object_materials"], cfg, golden_beams(P.LOOP_SAMPLES), P.loop_pose(pose),
                              n_angles=P.LOOP_ANGLES, want_f32=False)[0]
        clouds.append(detect_ref.detect_frame(img, theta_min=0.0, theta_inc=theta_inc, resolution=cfg.resolution, **P.LOOP_DET)[0])
    return clouds


def test_closed_loop_point_to_line_beats_point_to_point_on_the_oracles_images():
    a, b = loop_clouds()
    surf, counts = R.surface_points([a], **R.LOOP_SURFELS)
    assert counts[0, 1] == 0 and len(surf[0]) >= 10
    recs, _, _ = R.register([b], surf[0], None, P.LOOP_GATE, P.LOOP_ITERATIONS)
    p2p, _, _ = P.register([b], a, None, P.LOOP_GATE, P.LOOP_ITERATIONS)
    yaw_err, t_err = P.loop_errors(recs[0])
    yaw_p2p, t_p2p = P.loop_errors(p2p[0])
    print("closed loop on the oracle's images, %d surface points of %d points: point-to-line yaw error %.4f deg, translation error %.4f m, %d of %d matched; "
          "point-to-point %.4f deg, %.4f m" % (len(surf[0]), len(a), math.degrees(yaw_err), t_err, recs[0]["n_matched"], len(b), math.degrees(yaw_p2p), t_p2p))
    assert recs[0]["flags"] == 0
    assert yaw_err < yaw_p2p and t_err < t_p2p                        # the condition: better than point-to-point in both, on the same clouds
    # the constants are what is measured here, to the digits given
    assert abs(yaw_err - R.LOOP_YAW_MEASURED) <= math.radians(0.0001) and abs(t_err - R.LOOP_T_MEASURED) <= 1e-4


# ---- the layers above, the kernels, the documents --------------------------------------------------------------------------------------
def test_the_facade_has_the_calls_and_the_documents_name_them():
    assert callable(radar.RadarHIP.surfacePoints) and callable(radar.RadarHIP.registerSurfacePoints)
    assert "X_h T^-1" in radar.RadarHIP.registerSurfacePoints.__doc__
    readme, design, baseline, integ = (open(os.path.join(ROOT, f)).read() for f in ("README.md", "DESIGN.md", "BASELINE.md", "INTEGRATION.md"))
    for n in NEW:
        assert n in integ or n.replace("_device", "[_device]") in integ, n
    assert "registerSurfacePoints" in readme and "## 31." in design and "k_icp_pass<LineResidual>" in design and "## 28." in baseline


def test_surfel_kernels_use_no_scratch_and_the_lds_they_were_designed_for(native_lib):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    # the surface-point kernels are rr_surfels.hip's; the point-to-line matcher is rr_icp.hip's kernels instantiated for LineResidual
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-surfels", "resource-usage-icp"], capture_output=True, text=True, timeout=600)
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
    for k in ("k_sf_bin", "k_sf_decide", "k_sf_offsets", "k_sf_write"):
        assert k in names, (k, sorted(rows))
    for k in ("k_icp_init", "k_icp_pass", "k_icp_solve"):
        assert any(k in name and "LineResidual" in name for name in rows), (k, sorted(rows))
    _, tgt_tile = native_lib.icp_tile_sizes()
    for name, u in rows.items():
        assert u["scratch"] == 0, (name, u)
        scan = any(k in name for k in ("k_sf_decide", "k_sf_offsets", "k_sf_write"))
        assert u["lds"] == (8 * tgt_tile if "k_icp_pass" in name else 32 if scan else 0), (name, u)
        assert u["vgprs"] <= 128, (name, u)                            # four waves per SIMD at the least


def test_surfel_source_is_in_the_library_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rr_surfels.hip" in src
    assert re.search(r"^resource-usage-surfels:", mk, re.M)
