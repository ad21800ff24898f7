"""Translation registration without a GPU: the numpy restatement (tests/shift_ref.py) agrees with the literal slice definition
and with hand-worked cases, the feature's header text (names, prototypes and layouts: tests/test_abi.py), the wrappers
refuse bad arguments before any call into the library, the kernels of rr_shift.hip use no scratch and at most the LDS their
header states -- and the scene and the two poses of the simulated GPU test (tests/test_gpu_shift.py) are fixed here, where the
restatement alone, on the oracle's images, must land within one pixel."""
import os
import re
import subprocess

import numpy as np
import pytest

import detect_ref as Dr
import shift_ref as R
from common import golden_beams, mats_tuple
from radarays_ros_amd import native, params, radar, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radarays_ros_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "radarays_mi355.h")

# the simulated case: the 12-triangle room (20 m x 16 m), 200 cells of 0.1 m, noise off; Cartesian images of 128 x 128 pixels of
# 0.2 m; the image under test is rendered (-6, +4) pixels' worth of metres (forward, left) away from the reference's pose, at the
# same yaw, so its content is found at (dy, dx) = (+6, -4) in the reference
SIM = {"scene": scenes.box12, "n_samples": 50, "n_cells": 200, "width": 128, "pixel_size": 0.2, "max_shift": 8, "yaw": 0.3,
       "at": (1.0, 1.5, 0.2), "want": (6, -4),
       "cfg": lambda: params.kaist_preset(n_reflections=2, n_samples=50, ambient_noise=0, n_cells=200, resolution=0.1)}


def sim_poses():
    """(pose_x, pose_r): t_x - t_r = (-dy, -dx) * pixel_size in the sensor's (forward, left) axes"""
    yaw, ps, (dy, dx) = SIM["yaw"], SIM["pixel_size"], SIM["want"]
    fwd, left = np.array([np.cos(yaw), np.sin(yaw)]), np.array([-np.sin(yaw), np.cos(yaw)])
    t_r = np.array(SIM["at"][:2])
    t_x = t_r + (-dy * ps) * fwd + (-dx * ps) * left
    return scenes.yaw_pose(t_x[0], t_x[1], SIM["at"][2], yaw), scenes.yaw_pose(t_r[0], t_r[1], SIM["at"][2], yaw)


def pair(shape, seed):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, shape).astype(np.uint8), rs.randint(0, 256, shape).astype(np.uint8)


@pytest.mark.parametrize("shape", [(40, 37, 3), (100, 70, 32), (150, 200, 64)])
def test_restatement_equals_the_literal_definition_for_every_shift(shape):
    H, W, S = shape
    x, r = pair((H, W), H)
    lit = R.xcorr_literal(x, r, S)
    assert np.array_equal(R.xcorr(x, r, S), lit)
    # the box sums against literal slices, at the corners and the centre of the window of shifts
    Sr, Srr = R.box_sums(r, S)
    ri = r.astype(np.int64)
    for g, f in ((0, 0), (0, 2 * S), (2 * S, 0), (2 * S, 2 * S), (S, S), (S // 2, S + S // 3)):
        t = ri[g:g + H - 2 * S, f:f + W - 2 * S]
        assert Sr[g, f] == t.sum() and Srr[g, f] == (t * t).sum()
    # the SSE surface is the literal sum of squared differences
    got = R.shift(x, r, S, surface=lit)
    xt = x[S:H - S, S:W - S].astype(np.int64)
    for g, f in ((0, 0), (S, S), (2 * S, S // 2)):
        assert int(got["sse_surface"][g, f]) == int(((xt - ri[g:g + H - 2 * S, f:f + W - 2 * S]) ** 2).sum())


SINGLE = [(7, 5), (7, -5), (-7, 5), (-7, -5), (2, -9)]


@pytest.mark.parametrize("dy,dx", SINGLE)
def test_hand_worked_single_pixels(dy, dx):
    """x has one pixel of value 3 at (i0, j0), r one of value 5 at (i1, j1): 15 at (i1 - i0, j1 - j0), 0 elsewhere -- all four
    sign combinations, and one case with |dy| != |dx| so that a swapped row and column cannot hide"""
    H, W, S, i0, j0 = 50, 64, 10, 21, 30
    x, r = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    x[i0, j0], r[i0 + dy, j0 + dx] = 3, 5
    want = np.zeros((2 * S + 1, 2 * S + 1), np.int64)
    want[dy + S, dx + S] = 15
    assert np.array_equal(R.xcorr(x, r, S), want) and np.array_equal(R.xcorr_literal(x, r, S), want)
    got = R.shift(x, r, S)
    assert (got["dy"], got["dx"]) == (dy, dx) and got["n_best"] == 1 and got["xcorr"] == 15 and got["sse"] == 9 + 25 - 30
    assert (got["sum_x"], got["sum_xx"], got["sum_r"], got["sum_rr"]) == (3, 9, 5, 25)
    # a pixel of x outside T takes no part
    x2 = np.zeros((H, W), np.uint8)
    x2[S - 1, j0] = 3
    assert not R.xcorr(x2, r, S).any()


def test_a_cut_of_the_reference_is_found_where_it_was_cut():
    """x[T] = r[T + (p, q)]: no error is left at (p, q).  The sub-pixel offsets are what the definition's parabola gives for the
    neighbours' SSE -- with sse == 0 at the best shift that is 0.5 (e[-1] - e[+1]) / (e[-1] + e[+1]), at most half a pixel, and 0
    only where a neighbour lies outside the window of shifts (here: dy = -S) or the two neighbours happen to be equal"""
    H, W, S = 100, 70, 32
    _, r = pair((H, W), 5)
    for p, q in ((5, -11), (-S, 7)):
        x = np.roll(r, (-p, -q), axis=(0, 1))
        got = R.shift(x, r, S)
        assert (got["dy"], got["dx"]) == (p, q) and got["sse"] == 0 and got["n_best"] == 1 and got["psnr"] == np.inf and got["ncc"] == 1.0
        e = got["sse_nb"]
        assert got["sub_dx"] == 0.5 * float(e[2] - e[3]) / float(e[2] + e[3]) and abs(got["sub_dx"]) <= 0.5
        if p == -S:
            assert e[0] == R.U64_MAX and got["sub_dy"] == 0.0
        else:
            assert got["sub_dy"] == 0.5 * float(e[0] - e[1]) / float(e[0] + e[1]) and abs(got["sub_dy"]) <= 0.5
    # a symmetric valley has its bottom on the pixel
    assert R.sub_of(40, 0, 40) == 0.0 and R.sub_of(10, 10, 10) == 0.0 and R.sub_of(30, 10, 10) == 0.5


def test_shift_entry_points_are_declared_and_exported(native_lib):
    """(names, argument types and struct layouts: tests/test_abi.py, for the whole header)"""
    header = open(HEADER).read()
    assert "#define RR_ABI_VERSION 7" in header
    assert "typedef struct rr_shift_record" in header


def _unopened(n_cells=64, n_angles=16):
    o = native.Context.__new__(native.Context)
    o._h = None
    o._L = None
    o.cfg = params.RadarModelConfig(n_cells=n_cells)
    o.n_angles = n_angles
    return o


def test_wrappers_refuse_bad_arguments_before_the_library():
    o = _unopened()
    good, ref = np.zeros((2, 40, 37), np.uint8), np.zeros((40, 37), np.uint8)
    polar = np.zeros((64, 16), np.uint8)
    for h, w, s in ((0, 37, 0), (40, 8193, 3), (40, 37, -1), (40, 37, 65), (6, 37, 3), (40, 6, 3), (40, 37, 19), (4096, 2049, 0),
                    (40.0, 37, 3), (40, 37, "3"), (True, 37, 0), (40, 37, None)):
        with pytest.raises(ValueError):
            o.shift_images_device(1, 2, 1, h, w, s)
    assert native.shift_window(4096, 2048, 0) == (4096, 2048, 0) and native.shift_window(8192, 1152, 64) == (8192, 1152, 64)
    for s in (-1, 65, 19, 3.0, None):
        with pytest.raises(ValueError):
            o.shift_images(good, ref, s)
    for bad in (np.zeros((2, 39, 37), np.uint8), np.zeros((2, 40, 37), np.float32), np.zeros((2, 2, 40, 37), np.uint8)):
        with pytest.raises(ValueError):
            o.shift_images(bad, ref, 3)
    with pytest.raises(ValueError):
        o.shift_images(good, good, 3)
    with pytest.raises(ValueError):
        o.shift_images(good, ref.astype(np.int8), 3)
    for a in ((None, 2, 1), (1, 2, None), (1, 0, 1), (1, 65536, 1), (1, 2.0, 1)):
        with pytest.raises(ValueError):
            o.shift_images_device(*a, 40, 37, 3)
    for poses in (np.zeros((0, 7)), np.zeros((65, 7)), np.zeros((2, 6)), [["a"] * 7]):
        with pytest.raises(ValueError):
            o.simulate_batch_shift(poses, polar, 64, 0.5, 3)
    for width, ps, s in ((0, 0.5, 0), (8193, 0.5, 3), (64, 0.0, 3), (64, float("nan"), 3), (64, 0.5, 32), (64, 0.5, 65), (64, 0.5, -1), (4096, 0.5, 0)):
        with pytest.raises(ValueError):
            o.simulate_batch_shift(np.zeros((1, 7)), polar, width, ps, s)
    with pytest.raises(ValueError):
        o.simulate_batch_shift(np.zeros((1, 7)), np.zeros((2, 64, 16), np.uint8), 64, 0.5, 3)
    with pytest.raises(ValueError):
        o.simulate_batch_shift(np.zeros((1, 7)), np.zeros((64, 17), np.uint8), 64, 0.5, 3)


def test_radar_facade_and_its_cpp_twin_have_the_call():
    assert callable(radar.RadarHIP.registerTranslation) and callable(radar.RadarHIP.registerPose)
    hpp = open(os.path.join(ROOT, "include", "radarays_ros_amd", "RadarHIP.hpp")).read()
    marshal = open(os.path.join(ROOT, "include", "radarays_ros_amd", "marshal.hpp")).read()
    assert "registerTranslation" in hpp and "marshal::register_translation" in hpp
    assert "rr_shift_images" in marshal and "rr_polar_to_cartesian" in marshal


def test_cpp_twin_compiles_with_the_call(tmp_path):
    """the header-only C++ facade with registerTranslation instantiated (host compiler, no GPU: the program is not run)"""
    prog = tmp_path / "use.cpp"
    prog.write_text('#include "radarays_ros_amd/marshal.hpp"\n'
                    'bool use(rr_ctx* c, const uint8_t* px, std::vector<rr_shift_record>& out, std::vector<double>& corr) {\n'
                    '    return radarays_ros_amd::marshal::register_translation(c, 2, 64, [&](size_t k) { return px + 64 * k; }, px, 32, 0.5f, 3, true, out, &corr);\n'
                    '}\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(prog)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_shift_kernels_use_no_scratch_and_at_most_the_lds_their_header_states():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-shift"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    rows, cur = [], None
    for line in (r.stdout + r.stderr).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            rows.append(cur)
            continue
        for key, name in ((r"ScratchSize \[bytes/lane\]", "scratch"), (r"LDS Size \[bytes/block\]", "lds")):
            m = re.search(r"remark:\s+" + key + r": (\d+)", line)
            if m and cur is not None:
                cur[name] = int(m.group(1))
    head = open(os.path.join(CSRC, "rr_shift.hip")).read().split("#include")[0]
    for text in ("k_shift_gram 20,128 B at S > 32", "14,784 B at S <= 32", "k_shift_finish 3,080 B", "k_shift_box_rows 4,096 B",
                 "k_shift_box_cols and k_shift_sums none", "No kernel uses scratch"):
        assert text in head, text
    stated = {"k_shift_gramILi5ELi2E": 20128, "k_shift_gramILi3ELi4E": 14784, "k_shift_finish": 3080, "k_shift_box_rows": 4096,
              "k_shift_box_cols": 0, "k_shift_sums": 0}
    assert len(rows) == len(stated), [u["name"] for u in rows]
    for k, lds in stated.items():
        hit = [u for u in rows if k in u["name"]]
        assert len(hit) == 1, (k, [u["name"] for u in rows])
        assert hit[0]["scratch"] == 0 and hit[0]["lds"] <= lds, (k, hit[0])


def test_shift_source_is_in_the_library_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rr_shift.hip" in src
    assert re.search(r"^resource-usage-shift:", mk, re.M)
    assert "k_shift" not in open(os.path.join(CSRC, "rr_align.hip")).read()
    launch = open(os.path.join(CSRC, "rr_launch.h")).read()
    for name in ("launch_shift_box", "launch_shift_sums", "launch_shift_gram", "launch_shift_finish"):
        assert len(re.findall(r"\b%s\(" % name, launch)) == 1, name


def test_the_simulated_case_lands_within_a_pixel_on_the_cpu(oracle):
    """the scene and the two poses of tests/test_gpu_shift.py's simulated case, through the oracle, the Cartesian restatement
    (tests/detect_ref.py) and the restatement of the registration alone: within one pixel of (+6, -4) on each axis"""
    O = oracle
    s = SIM["scene"]()
    cfg = SIM["cfg"]()
    sc = O.Scene(s["verts"], s["faces"], s["face_object_id"], use_bvh=0)
    beams = golden_beams(SIM["n_samples"])
    polar = [O.simulate(sc, mats_tuple(params.kaist_materials()), s["object_materials"], cfg, beams, p)[0] for p in sim_poses()]
    assert polar[0].shape == (SIM["n_cells"], 400) and polar[1].any()
    g = native.make_config(cfg, 400)
    cart = [Dr.cartesian(im, SIM["width"], SIM["pixel_size"], True, scroll=g.scroll_image, theta_min=g.theta_min, theta_inc=g.theta_inc,
                         resolution=g.resolution) for im in polar]
    got = R.shift(cart[0], cart[1], SIM["max_shift"])
    print("cpu: (dy, dx) = (%d, %d) sub (%.3f, %.3f) sse %d ncc %.6f n_best %d" % (got["dy"], got["dx"], got["sub_dy"], got["sub_dx"], got["sse"],
                                                                                  got["ncc"], got["n_best"]))
    assert abs(got["dy"] - SIM["want"][0]) <= 1 and abs(got["dx"] - SIM["want"][1]) <= 1
    assert got["n_best"] == 1
