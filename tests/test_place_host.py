"""Place recognition without a GPU: the numpy restatement (tests/place_ref.py) agrees with the literal definitions and with
hand-worked cases, the feature's header text is as stated (names, prototypes and layouts: tests/test_abi.py), the wrappers refuse bad
arguments before any call into the library, the kernels of rr_place.hip use no scratch and at most the LDS their header states --
and the scene, the 12 database poses and the query of the simulated GPU test (tests/test_gpu_place.py) are fixed here, where the
restatement alone, on the oracle's images, must put the right pose first."""
import os
import re
import subprocess

import numpy as np
import pytest

import place_ref as R
from common import golden_beams, mats_tuple
from radarays_ros_amd import native, params, radar, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radarays_ros_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "radarays_mi355.h")
NEW = ["rr_describe_images_device", "rr_describe_images", "rr_simulate_batch_describe", "rr_match_descriptors_device", "rr_match_descriptors"]

# the simulated case: the 12-triangle room (20 m x 16 m), 200 cells of 0.1 m, noise off; descriptors of 10 rings x 40 sectors (10
# image columns per sector); 12 database poses on a 4 x 3 grid whose |x| and |y| are all different, so that no two are images of
# each other under the room's mirror symmetries; the query is pose 5 turned by 7 sectors' worth of yaw
SIM = {"scene": scenes.box12, "n_samples": 50, "n_cells": 200, "R": 10, "S": 40, "yaw": 0.3, "z": 0.2, "hit": 5, "sectors": 7,
       "xs": (-6.3, -2.1, 1.9, 5.2), "ys": (-4.4, -0.9, 3.1),
       "cfg": lambda: params.kaist_preset(n_reflections=2, n_samples=50, ambient_noise=0, n_cells=200, resolution=0.1)}
# the shift at which a query is found whose pose is the database pose turned by SIM["sectors"] sectors along the sweep, a yaw of
# sectors * (n_angles / S) * theta_inc with theta_inc = -2 pi / n_angles.  Settled by the CPU test below: the shift is +sectors.
# It is the QUERY's image that the shift moves, so by the rule RadarHIP.registerPose uses for an azimuth shift the query's pose
# turned by -s * (n_angles / S) * theta_inc is the candidate's, and the candidate's turned by +s * (n_angles / S) * theta_inc the query's
SIM_SHIFT = SIM["sectors"]


def sim_database_poses():
    return np.stack([scenes.yaw_pose(x, y, SIM["z"], SIM["yaw"]) for y in SIM["ys"] for x in SIM["xs"]])


def sim_query_pose():
    p = sim_database_poses()[SIM["hit"]]
    turn = SIM["sectors"] * (400 // SIM["S"]) * (-2.0 * np.pi / 400.0)       # sectors * (n_angles / S) * theta_inc
    return scenes.yaw_pose(p[4], p[5], p[6], SIM["yaw"] + turn)


def pair(R_, S_, n, seed):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, (R_, S_)).astype(np.uint8), rs.randint(0, 256, (n, R_, S_)).astype(np.uint8)


@pytest.mark.parametrize("shape", [(3, 5), (20, 60), (64, 128)])
def test_restatement_equals_the_literal_roll_for_every_shift(shape):
    q, db = pair(shape[0], shape[1], 3, shape[1])
    xc = R.xcorr(q, db)
    assert xc.shape == (shape[1], 3)
    for i in range(3):
        assert np.array_equal(xc[:, i], R.xcorr_roll(q, db[i]))
    rec, sse, shift = R.match(q[None], db, 3)
    for i in range(3):
        lit = R.xcorr_roll(q, db[i])
        s = int(np.argmax(lit))
        d = np.roll(q, s, axis=1).astype(np.int64) - db[i].astype(np.int64)
        assert int(shift[0, i]) == s and int(sse[0, i]) == int((d * d).sum())          # the SSE is the literal sum of squared differences
    assert [r["sse"] for r in rec[0]] == sorted(int(v) for v in sse[0])


@pytest.mark.parametrize("case", [(200, 37, 3, 197, 7, 5), (3424, 400, 0, 3424, 20, 60)])
def test_descriptor_restatement_equals_a_literal_double_loop(case):
    n_cells, n_angles, cb, ce, R_, S_ = case
    img = np.random.RandomState(n_angles).randint(0, 256, (n_cells, n_angles)).astype(np.uint8)
    d = R.describe(img, cb, ce, R_, S_)
    assert d.dtype == np.uint8 and d.shape == (R_, S_)
    assert np.array_equal(d, R.describe_literal(img, cb, ce, R_, S_))
    # every column lies in the sector the kernel's closed form gives: floor(((a + 1) S - 1) / A)
    edges = R.sector_edges(n_angles, S_)
    for a in range(n_angles):
        j = ((a + 1) * S_ - 1) // n_angles
        assert edges[j] <= a < edges[j + 1]
    assert np.all(R.describe(np.full((n_cells, n_angles), 255, np.uint8), cb, ce, R_, S_) == 255)


@pytest.mark.parametrize("j0,j1", [(3, 11), (11, 3)])
def test_hand_worked_single_cells(j0, j1):
    """q holds 3 at (r0, j0), c holds 5 at (r0, j1): 15 at s = (j1 - j0) mod S only -- once with j1 < j0"""
    R_, S_, r0 = 6, 17, 4
    q, c = np.zeros((R_, S_), np.uint8), np.zeros((R_, S_), np.uint8)
    q[r0, j0], c[r0, j1] = 3, 5
    want = np.zeros(S_, np.int64)
    want[(j1 - j0) % S_] = 15
    assert np.array_equal(R.xcorr_roll(q, c), want) and np.array_equal(R.xcorr(q, c[None])[:, 0], want)
    rec, sse, shift = R.match(q[None], c[None], 1)
    assert rec[0][0] == {"index": 0, "shift": (j1 - j0) % S_, "sse": 9 + 25 - 30, "n_best": 1, "xcorr": 15, "ncc": rec[0][0]["ncc"],
                         "psnr": rec[0][0]["psnr"]}
    # the same values in different rings never meet
    c2 = np.zeros((R_, S_), np.uint8)
    c2[r0 - 1, j1] = 5
    assert not R.xcorr(q, c2[None]).any() and not R.xcorr_roll(q, c2).any()
    rec, _, _ = R.match(q[None], c2[None], 1)
    assert rec[0][0]["n_best"] == S_ and rec[0][0]["shift"] == 0 and rec[0][0]["sse"] == 34


def test_constants_tie_on_every_shift_and_duplicates_come_in_index_order():
    R_, S_ = 5, 12
    q = np.full((R_, S_), 9, np.uint8)
    rec, sse, shift = R.match(q[None], np.full((2, R_, S_), 200, np.uint8), 2)
    for k in (0, 1):
        assert rec[0][k]["n_best"] == S_ and rec[0][k]["shift"] == 0 and rec[0][k]["ncc"] == 0.0 and rec[0][k]["index"] == k
    q, db = pair(R_, S_, 6, 2)
    db[4] = db[1] = np.roll(q, 5, axis=1)
    rec, sse, shift = R.match(q[None], db, 3)
    assert [r["index"] for r in rec[0][:2]] == [1, 4] and all(r["sse"] == 0 and r["shift"] == 5 and r["ncc"] == 1.0 for r in rec[0][:2])
    assert rec[0][0]["psnr"] == np.inf and rec[0][2]["sse"] > 0


def test_place_entry_points_are_declared_and_exported(native_lib):
    """(names, argument types and struct layouts: tests/test_abi.py, for the whole header)"""
    header = open(HEADER).read()
    assert "#define RR_ABI_VERSION 7" in header
    assert "typedef struct rr_place_match" in header and "typedef struct rr_place_config" in header
    assert "unpinned" in header.split("typedef struct rr_place_config")[0].split("place recognition")[-1]


def _unopened(n_cells=64, n_angles=16):
    o = native.Context.__new__(native.Context)
    o._h = None
    o._L = None
    o.cfg = params.RadarModelConfig(n_cells=n_cells)
    o.n_angles = n_angles
    return o


def test_wrappers_refuse_bad_arguments_before_the_library():
    o = _unopened()
    imgs = np.zeros((2, 64, 16), np.uint8)
    for bad in ((0, 8), (65, 8), (4, 3), (4, 129), (4, 17), (65, 128), (4.0, 8), (4, "8"), (True, 8), (4, 8, -1), (4, 8, 0, 65), (4, 8, 10, 10),
                (8, 8, 10, 17), {"n_rings": 4, "n_sectors": 8, "cell_begin": 3, "cell_end": 2}, (4, 8, 0.0, 64)):
        with pytest.raises(ValueError):
            o.describe_images(imgs, bad)
        with pytest.raises(ValueError):
            o.describe_images_device(1, 2, bad, 1)
        with pytest.raises(ValueError):
            o.simulate_batch_describe(np.zeros((1, 7)), bad)
    c = native.place_config(64, 128, 3424, 400)
    assert (c.cell_begin, c.cell_end, c.n_rings, c.n_sectors) == (0, 3424, 64, 128)
    assert native.place_shape(64, 128) == (64, 128)
    with pytest.raises(ValueError):
        native.place_shape(64, 129)
    with pytest.raises(ValueError):
        native.place_config(20, 60, 3424, 59)
    for bad in (np.zeros((2, 64, 17), np.uint8), np.zeros((2, 64, 16), np.float32)):
        with pytest.raises(ValueError):
            o.describe_images(bad, (4, 8))
    for a in ((None, 2, (4, 8), 1), (1, 2, (4, 8), None), (1, 0, (4, 8), 1), (1, 65536, (4, 8), 1)):
        with pytest.raises(ValueError):
            o.describe_images_device(*a)
    for poses in (np.zeros((0, 7)), np.zeros((65, 7)), np.zeros((2, 6))):
        with pytest.raises(ValueError):
            o.simulate_batch_describe(poses, (4, 8))
    q, db = np.zeros((2, 4, 8), np.uint8), np.zeros((5, 4, 8), np.uint8)
    for k in (0, 6, 33, 2.0, None, True):
        with pytest.raises(ValueError):
            o.match_descriptors(q, db, k)
    for bq, bd in ((q.astype(np.int8), db), (q, db.astype(np.float32)), (q, np.zeros((5, 4, 9), np.uint8)), (q, db[0]), (np.zeros((65, 4, 8), np.uint8), db),
                   (np.zeros((2, 4, 3), np.uint8), np.zeros((5, 4, 3), np.uint8)), (np.zeros((2, 65, 4), np.uint8), np.zeros((5, 65, 4), np.uint8)),
                   (q, np.zeros((0, 4, 8), np.uint8))):
        with pytest.raises(ValueError):
            o.match_descriptors(bq, bd, 1)
    for a in ((None, 2, 1, 5, 4, 8, 1), (1, 2, None, 5, 4, 8, 1), (1, 0, 1, 5, 4, 8, 1), (1, 65, 1, 5, 4, 8, 1), (1, 2, 1, 0, 4, 8, 1),
              (1, 2, 1, (1 << 28) + 1, 4, 8, 1), (1, 2, 1, 5, 4, 8, 6), (1, 2, 1, 50, 4, 8, 33), (1, 2, 1, 5, 65, 4, 1), (1, 2, 1, 5, 4, 3, 1),
              (1, 2, 1, 5, 64, 129, 1), (1, 2, 1, 5, 65, 128, 1)):
        with pytest.raises(ValueError):
            o.match_descriptors_device(*a)
    with pytest.raises(ValueError):
        o.match_descriptors_device(1, 2, 1, 5, 4, 8, 1, d_shift_ptr=1)


def test_radar_facade_and_its_cpp_twin_have_the_calls():
    assert callable(radar.RadarHIP.buildPlaceDatabase) and callable(radar.RadarHIP.localize)
    hpp = open(os.path.join(ROOT, "include", "radarays_ros_amd", "RadarHIP.hpp")).read()
    marshal = open(os.path.join(ROOT, "include", "radarays_ros_amd", "marshal.hpp")).read()
    assert "describeImages" in hpp and "localize" in hpp and "marshal::describe" in hpp and "marshal::match_places" in hpp
    assert "rr_describe_images" in marshal and "rr_match_descriptors" in marshal


def test_cpp_twin_compiles_with_the_calls(tmp_path):
    """the header-only C++ marshalling with describe and match_places instantiated (host compiler, no GPU: the program is not run)"""
    prog = tmp_path / "use.cpp"
    prog.write_text('#include "radarays_ros_amd/marshal.hpp"\n'
                    'bool use(rr_ctx* c, const uint8_t* px, std::vector<uint8_t>& d, std::vector<rr_place_match>& out) {\n'
                    '    rr_place_config p{0, 8, 2, 4};\n'
                    '    return radarays_ros_amd::marshal::describe(c, 2, 64, [&](size_t k) { return px + 64 * k; }, p, d) &&\n'
                    '           radarays_ros_amd::marshal::match_places(c, d.data(), 1, d.data(), 2, 2, 4, 1, out);\n'
                    '}\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(prog)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_place_kernels_use_no_scratch_and_at_most_the_lds_their_header_states():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-place"], capture_output=True, text=True, timeout=600)
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
    head = open(os.path.join(CSRC, "rr_place.hip")).read().split("#include")[0]
    for text in ("k_place_match 8,960 B", "k_place_describe 1,024 B", "k_place_rolls 32 B", "k_place_topk 32 B", "k_place_gather and k_place_finish none",
                 "No kernel uses scratch"):
        assert text in head, text
    stated = {"k_place_matchILb1E": 8960, "k_place_matchILb0E": 8960, "k_place_describeILi16E": 1024, "k_place_describeILi1E": 1024, "k_place_rolls": 32,
              "k_place_topk": 32, "k_place_gather": 0, "k_place_finish": 0}
    assert len(rows) == len(stated), [u["name"] for u in rows]
    for k, lds in stated.items():
        hit = [u for u in rows if k in u["name"]]
        assert len(hit) == 1, (k, [u["name"] for u in rows])
        assert hit[0]["scratch"] == 0 and hit[0]["lds"] <= lds, (k, hit[0])


def test_place_source_is_in_the_library_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rr_place.hip" in src
    assert re.search(r"^resource-usage-place:", mk, re.M)
    for other in ("rr_align.hip", "rr_shift.hip"):
        assert "k_place" not in open(os.path.join(CSRC, other)).read()
    launch = open(os.path.join(CSRC, "rr_launch.h")).read()
    for name in ("launch_place_describe", "launch_place_rolls", "launch_place_match", "launch_place_topk", "launch_place_finish"):
        assert len(re.findall(r"\b%s\(" % name, launch)) == 1, name
    images = open(os.path.join(CSRC, "rr_images.hip")).read()
    for n in NEW:
        assert re.search(r"^int %s\(" % n, images, re.M), n


def test_the_simulated_case_puts_the_right_pose_first_on_the_cpu(oracle):
    """the scene, the 12 poses and the query of tests/test_gpu_place.py's simulated case, through the oracle and the restatement
    alone: index 5 first, n_best == 1, the shift the turn dictates, a strictly larger SSE for rank 2"""
    O = oracle
    s = SIM["scene"]()
    cfg = SIM["cfg"]()
    sc = O.Scene(s["verts"], s["faces"], s["face_object_id"], use_bvh=0)
    beams = golden_beams(SIM["n_samples"])
    mats = mats_tuple(params.kaist_materials())
    poses = list(sim_database_poses()) + [sim_query_pose()]
    assert len(poses) == 13
    imgs = [O.simulate(sc, mats, s["object_materials"], cfg, beams, p)[0] for p in poses]
    assert imgs[0].shape == (SIM["n_cells"], 400) and all(im.any() for im in imgs)
    desc = np.stack([R.describe(im, 0, SIM["n_cells"], SIM["R"], SIM["S"]) for im in imgs])
    rec, sse, shift = R.match(desc[12:], desc[:12], 3)
    print("cpu:", [(r["index"], r["shift"], r["sse"], r["n_best"], round(r["ncc"], 4)) for r in rec[0]])
    first, second = rec[0][0], rec[0][1]
    assert first["index"] == SIM["hit"] and first["n_best"] == 1 and first["shift"] == SIM_SHIFT
    assert second["sse"] > first["sse"]
    # no two database entries are alike: the mirror images of the room are not in the database
    assert len({d.tobytes() for d in desc[:12]}) == 12
