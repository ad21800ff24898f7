"""Echo provenance without a GPU: the numpy restatement of the label definition (tests/labels_ref.py) on hand-worked cases, the new
constants and header text of the feature (names, prototypes and the record layout: tests/test_abi.py) -- and the scene, config and poses of the GPU tests
(tests/test_gpu_labels.py) fixed here together with the premises those tests rest on, checked on the oracle."""
import os
import re

import numpy as np
import pytest

import labels_ref as R
from common import golden_beams, mats_tuple
from radarays_ros_amd import native, params, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "radarays_mi355.h")
N_ANGLES = 400

# ---- the simulated case ---------------------------------------------------------------------------------------------------------
# object 0: a box of half-size 5 m around the origin with its +x wall removed (10 triangles, faces 0..9), penetrable material;
# object 1: a closed box of half-size 12 m around it (faces 10..21), the KAIST wall.  From a sensor within 0.3 m of the origin the
# pass-0 ranges of object 0 lie in [4.7, 9.2] m and those of object 1 in [11.7, 21.3] m: 512 cells of 0.05 m put both inside the image
NEAR_BAND = (int(4.5 / 0.05), int(9.5 / 0.05))          # cells [90, 190]
FAR_BAND = (int(11.0 / 0.05), int(21.5 / 0.05))         # cells [220, 430]
POSES = [scenes.yaw_pose(0.0, 0.0, 0.0, 0.3), scenes.yaw_pose(0.25, -0.2, 0.1, 1.1)]
POSE3 = POSES + [scenes.yaw_pose(-0.2, 0.3, -0.1, 2.0)]


def scene():
    v0, f0 = scenes._box_tris([-5, -5, -5], [5, 5, 5])
    f0 = np.array([f for f in f0 if not all(v0[i, 0] == 5 for i in f)], np.uint32)          # the +x wall goes
    assert len(f0) == 10
    v1, f1 = scenes._box_tris([-12, -12, -12], [12, 12, 12], vbase=8)
    return {"verts": np.concatenate([v0, v1]), "faces": np.concatenate([f0, f1]),
            "face_object_id": np.concatenate([np.zeros(10, np.uint32), np.ones(12, np.uint32)]), "object_materials": [2, 1], "name": "nested_boxes"}


def materials():
    return params.kaist_materials() + [params.PENETRABLE]          # air, wall stone (opaque), v = 0.1 (refracts)


def config(n_reflections=3, record_multi_path=False, scroll_image=0):
    return params.kaist_preset(n_cells=512, resolution=0.05, n_samples=24, n_reflections=n_reflections, ambient_noise=0, signal_denoising=1,
                               signal_denoising_triangular_width=9, record_multi_path=record_multi_path, scroll_image=scroll_image)


def beams():
    return golden_beams(24)


def through_the_opening(pose):
    """azimuths whose heading in the map lies within 30 degrees of +x: every beam sample (10 degree cone) leaves through the opening"""
    yaw = 2.0 * np.arctan2(float(pose[2]), float(pose[3]))
    head = yaw + np.arange(N_ANGLES) * (-2.0 * np.pi / N_ANGLES)
    return np.abs(np.angle(np.exp(1j * head))) < np.radians(30.0)


def oracle_log(oracle, pose, **cfg_kw):
    s = scene()
    sc = oracle.Scene(s["verts"], s["faces"], s["face_object_id"], use_bvh=0)
    log = {"cap": 1024}
    u8, f32, st = oracle.simulate(sc, mats_tuple(materials()), s["object_materials"], config(**cfg_kw), beams(), pose, echo_log=log)
    assert log["counts"].max() <= 1024
    return u8, st, log


_LOGS = {}


def logged(oracle, pose_index, n_reflections, rmp):
    """the oracle's image, stats and echo log of one pose / config of the GPU tests, computed once"""
    key = (pose_index, n_reflections, bool(rmp))
    if key not in _LOGS:
        _LOGS[key] = oracle_log(oracle, POSE3[pose_index], n_reflections=n_reflections, record_multi_path=rmp)
    return _LOGS[key]


# ---- the restatement on hand-worked cases -----------------------------------------------------------------------------------------
TRI5 = np.float32([0.0, 0.5, 1.0, 0.5, 0.25])          # W = 5, mode = 2: an echo at cell c reaches bins c - 2 .. c + 2


def cols(cells, strs, infos=None, faces=None, n_cells=16, w=TRI5, mode=2):
    n = len(cells)
    infos = np.arange(100, 100 + n, dtype=np.uint32) if infos is None else infos
    faces = np.arange(500, 500 + n, dtype=np.uint32) if faces is None else faces
    a = R.label_column(cells, np.float32(strs), infos, faces, n_cells, w, mode)
    b = R.label_column_fast(cells, np.float32(strs), infos, faces, n_cells, w, mode)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    return a


def test_a_single_echo_labels_its_window_where_the_weight_is_positive():
    lab, fac = cols([8], [2.0])
    want = np.full(16, R.NONE, np.uint32)
    want[7:11] = 100                         # bins 7 .. 10: weights 0.5 1 0.5 0.25; bin 6 has weight 0 -> a zero term never wins
    assert np.array_equal(lab, want) and np.array_equal(fac, np.where(want == 100, 500, R.NONE))


def test_equal_terms_go_to_the_first_echo_and_a_larger_term_wins_whatever_its_place():
    lab, _ = cols([8, 8], [2.0, 2.0])
    assert set(lab[7:11]) == {100}
    lab, _ = cols([8, 8, 8], [2.0, 3.0, 3.0])
    assert set(lab[7:11]) == {101}
    # 1.0 * w[mode] = 1 from cell 9 against 2.0 * 0.5 = 1 from cell 8, both on bin 9: equal terms, the first echo keeps the bin
    lab, _ = cols([8, 9], [2.0, 1.0])
    assert lab[9] == 100 and lab[10] == 100          # bin 10: 0.5 from cell 8 (tap 4: 0.25 * 2) against 0.5 (tap 3: 0.5 * 1): first again
    assert lab[11] == 101                            # ... and bin 11 is reached by the second echo alone
    lab, _ = cols([9, 8], [1.0, 2.0])
    assert lab[9] == 100 and lab[8] == 101


def test_windows_are_clipped_at_bin_1_and_at_the_last_bin():
    lab, _ = cols([1], [1.0])                # window -1 .. 3: bins -1 and 0 are outside (bin 0 is never written)
    assert lab[0] == R.NONE and list(lab[1:4]) == [100, 100, 100] and lab[4] == R.NONE
    lab, _ = cols([0], [1.0])                # its mode tap falls on bin 0: only taps 3, 4 land
    assert lab[0] == R.NONE and list(lab[1:3]) == [100, 100] and lab[3] == R.NONE
    lab, _ = cols([15], [1.0])               # window 13 .. 17: bins 16, 17 do not exist; bin 13 has weight 0
    assert list(lab[13:16]) == [R.NONE, 100, 100]


def test_echoes_beyond_the_image_are_dropped():
    lab, _ = cols([16, 17, -1, 40], [9.0, 9.0, 9.0, 9.0])          # cell 16's window would reach bins 14, 15
    assert (lab == R.NONE).all()


@pytest.mark.parametrize("bad", [-3.0, 0.0, -0.0, np.inf, -np.inf, np.nan])
def test_a_term_that_is_not_finite_and_positive_never_wins(bad):
    lab, _ = cols([8], [bad])
    assert (lab == R.NONE).all()
    lab, _ = cols([8, 8, 8], [bad, 1e-30, bad])
    assert set(lab[7:11]) == {101}


def test_without_a_denoiser_an_echo_labels_its_own_bin():
    one = np.ones(1, np.float32)
    lab, fac = cols([3, 3, 0, 15, 7], [1.0, 2.0, 5.0, 1.0, 4.0], w=one, mode=0)
    want = np.full(16, R.NONE, np.uint32)
    want[3], want[15], want[7] = 101, 103, 104          # (bin 0 stays unlabelled)
    assert np.array_equal(lab, want)


def test_the_term_is_the_f64_product_rounded_once():
    s, w = np.float32(1.0 + 2.0 ** -23), np.float32(1.0 - 2.0 ** -24)
    assert R.term(s, w) == np.float32(np.float64(s) * np.float64(w))
    w3 = np.float32([0.0, w, 1.0])
    lab, _ = cols([8, 7], [s, 1.0], w=w3, mode=2)          # bin 7: s * w (tap 1 of cell 8) against 1.0 (tap 2 of cell 7)
    assert lab[7] == (100 if R.term(s, w) >= np.float32(1.0) else 101)


def test_info_word_round_trip():
    for obj, pas, kind in ((0, 0, 0), (5, 2, 1), (0xFFFFFE, 15, 1)):
        o, p, k = native.unpack_info(R.pack_info(obj, pas, kind))
        assert (int(o), int(p), int(k)) == (obj, pas, kind)
    o, p, k = native.unpack_info(np.array([R.pack_info(3, 1, 0), R.pack_info(4, 0, 1)], np.uint32))
    assert list(o) == [3, 4] and list(p) == [1, 0] and list(k) == [0, 1]
    from radarays_ros_amd import radar
    assert radar.unpack_info is native.unpack_info and hasattr(radar.RadarHIP, "simulate_provenance")


# ---- header, library and binding --------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound(native_lib):
    """(names, argument types and struct layouts: tests/test_abi.py, for the whole header)"""
    header = open(HEADER).read()
    assert "#define RR_ABI_VERSION 7" in header
    assert "#define RR_LABEL_NONE 0xFFFFFFFFu" in header and native_lib.LABEL_NONE == 0xFFFFFFFF == R.NONE
    m = re.search(r"#define RR_LABEL_MAX_CELLS (\d+)", header)
    assert m and int(m.group(1)) == native_lib.LABEL_MAX_CELLS >= 8192
    section = header.split("---- echo provenance")[1].split("typedef struct rr_echo_src")[0]
    assert "UNPINNED" in section and "may still render 0" in section and "0xFFFFFFFF - k" in section


def test_calls_without_a_context_or_config_are_refused(native_lib):
    L = native_lib.lib()
    assert L.rr_simulate_batch_provenance_device(None, None, 1, None, None, None, None, 0, None, None) == -1
    assert L.rr_simulate_provenance(None, None, None, None, None, None, 0, None) == -1
    assert L.rr_debug_labels(None, 1, 0, None, None, 0, None, None) == -1


# ---- the premises of the GPU tests, on the oracle ------------------------------------------------------------------------------
def test_scene_has_two_objects_and_an_opening():
    s = scene()
    assert len(s["faces"]) == 22 and s["faces"].max() < len(s["verts"]) == 16
    assert through_the_opening(POSES[0]).sum() in range(60, 70)           # 60 degrees of 360: 66 or 67 of 400 azimuths


@pytest.mark.parametrize("rmp", [False, True], ids=["path", "multipath"])
@pytest.mark.parametrize("pose_index", [0, 1, 2])
def test_premises_of_the_gpu_tests(oracle, pose_index, rmp):
    """(a) the stream at n_reflections = P begins with the stream at P - 1; (b) no wave energy within 1e-6 of the pruning threshold,
    where the last ulp of acosf decides a wave's fate; (c) every pass-0 echo lies in one of the two range bands"""
    logs = [logged(oracle, pose_index, P, rmp) for P in (1, 2, 3)]
    for u8, st, log in logs:
        assert st["near_threshold"] == 0, (pose_index, rmp, st)                           # (b)
    for (_, _, lo), (_, _, hi) in zip(logs[:-1], logs[1:]):                                # (a)
        assert (lo["counts"] <= hi["counts"]).all()
        for a in range(N_ANGLES):
            n = int(lo["counts"][a])
            assert np.array_equal(lo["cells"][a, :n], hi["cells"][a, :n]) and np.array_equal(lo["strengths"][a, :n], hi["strengths"][a, :n]), a
    one = logs[0][2]
    assert (logs[2][2]["counts"] > one["counts"]).any()                                   # later passes do echo
    for a in range(N_ANGLES):                                                              # (c)
        c = one["cells"][a, :int(one["counts"][a])]
        near = (c >= NEAR_BAND[0]) & (c <= NEAR_BAND[1])
        far = (c >= FAR_BAND[0]) & (c <= FAR_BAND[1])
        assert (near | far).all(), (a, c)
        if through_the_opening(POSE3[pose_index])[a]:
            assert far.all() and len(c) == 24, a
    if rmp:
        assert (logs[2][2]["counts"] > logged(oracle, pose_index, 3, False)[2]["counts"]).any()      # multipath echoes exist
