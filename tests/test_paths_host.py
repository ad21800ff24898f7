"""Wave paths without a GPU: the constants of include/radarays_mi355.h ("wave paths"; names, prototypes and
the record layout: tests/test_abi.py), the numpy helpers of
radarays_ros_amd/radar.py on hand-made lists, and the restatement of the bounce loop (tests/paths_ref.py) pinned to the oracle's
extended echo log -- exactly -- on eight azimuths of each case: the nested boxes of tests/test_gpu_labels.py ("N") and the cases A,
B and B2 of tests/test_stream_host.py.  The premises tests/test_gpu_paths.py rests on are proven here on the oracle alone.

Mutation note (scratch copies only, nothing committed).  In the restatement, swapping `branch` (2 for the reflection child, 1 for the
transmission child) and, separately, taking `parent` from the child slot s = 2 * i + branch - 1 instead of s >> 1 each turn every case
of test_restatement_is_consistent red (check_list: a parent outside the previous pass; the children of one parent out of branch
order).  tests/test_gpu_paths.py applies the same check_list to the kernel's lists and compares parent and info with the restatement
field by field, so the same two slips in k_wave_gather fail there; those kernel mutations were reasoned, not run."""
import os

import numpy as np
import pytest

import paths_ref as R
import test_labels_host as L
import test_stream_host as S
from common import mats_tuple
from radarays_ros_amd import radar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ANGLES = 400
AZS = (0, 1, 100, 101, 200, 201, 300, 301)
CASES = ("N", "A", "B", "B2")
RUNS = [("N", False), ("N", True), ("A", True), ("B", True), ("B2", True)]
IDS = ["%s-%s" % (c, "multipath" if m else "path") for c, m in RUNS]


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def scene(case):
    return L.scene() if case == "N" else S.scene(case)


def materials(case):
    return L.materials() if case == "N" else S.materials(case)


def config(case, rmp):
    return L.config(3, rmp) if case == "N" else S.config(case, rmp)


def beams(case):
    return L.beams() if case == "N" else S.beams(case)


def pose(case):
    return L.POSE3[0] if case == "N" else S.pose(case)


def n_passes(case):
    return 3 if case == "N" else S.n_reflections(case)


def logged(oracle, case, rmp):
    """(stats, extended echo log) of the oracle"""
    if case != "N":
        _, st, log = S.logged(oracle, case, rmp)
        return st, log
    key = ("paths", bool(rmp))
    if key not in L._LOGS:
        s = scene("N")
        sc = oracle.Scene(s["verts"], s["faces"], s["face_object_id"], use_bvh=0)
        log = {"cap": 1024}
        _, _, st = oracle.simulate(sc, mats_tuple(materials("N")), s["object_materials"], config("N", rmp), beams("N"), pose("N"), echo_log=log)
        L._LOGS[key] = (None, st, log)
    return L._LOGS[key][1:]


_REF = {}


def reference(oracle, case, rmp, az, map_frame=False):
    """paths_ref.trace_azimuth of one azimuth of a case, computed once: (waves, pass_counts, echoes), read-only"""
    key = (case, bool(rmp), int(az), bool(map_frame))
    if key not in _REF:
        s = scene(case)
        sk = ("scene", case)
        if sk not in _REF:
            _REF[sk] = oracle.Scene(s["verts"], s["faces"], s["face_object_id"], use_bvh=0 if case in ("N", "A") else 1)
        out = R.trace_azimuth(oracle, _REF[sk], s, mats_tuple(materials(case)), s["object_materials"], config(case, rmp), beams(case),
                              pose(case), az, N_ANGLES, map_frame)
        for v in out:
            v.setflags(write=False)
        _REF[key] = out
    return _REF[key]


# ---- the interface ------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound(native_lib):
    """(names, argument types and the record layout: tests/test_abi.py, for the whole header)"""
    header = open(os.path.join(ROOT, "include", "radarays_mi355.h")).read()
    assert "#define RR_ABI_VERSION 7" in header and native_lib.lib().rr_abi_version() == 7          # purely additive
    assert native_lib.WAVES_MAP_FRAME == 1 and "#define RR_WAVES_MAP_FRAME 1u" in header
    assert native_lib.WAVES_MAX_PASSES == 16 and "#define RR_WAVES_MAX_PASSES 16" in header


def test_calls_without_a_context_are_refused(native_lib):
    Lb = native_lib.lib()
    assert Lb.rr_simulate_batch_paths_device(None, None, 1, None, None, 0, None, None, 0, None) == -1
    assert Lb.rr_simulate_paths(None, None, None, None, 0, None, None, 0) == -1


# ---- the helpers --------------------------------------------------------------------------------------------------------------------
def hand_made(native_lib):
    """two beams; beam 0 hits (echo 0), reflects (wave 2: hits, both echoes 1 and 2) and transmits (wave 3: misses); beam 1 misses;
    wave 2 reflects into wave 4, which hits without an echo"""
    w = np.zeros(5, native_lib.WAVE_DTYPE)
    w["parent"], w["echo"], w["face"], w["range"] = [-1, -1, 0, 0, 2], [0, -1, 1, -1, -1], [7, 0xFFFFFFFF, 8, 0xFFFFFFFF, 9], [2.0, -1.0, 1.0, -1.0, 4.0]
    w["o"] = [[0, 0, 0], [0, 0, 0], [2, 0, 0.5], [2.5, 0, 0], [2, 1, 0.5]]
    w["d"] = [[1, 0, 0], [0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, -1]]
    info = lambda obj, p, br, e0, e1: obj | p << 24 | br << 28 | e0 << 30 | e1 << 31   # noqa: E731
    w["info"] = [info(3, 0, 0, 1, 0), info(0xFFFFFF, 0, 0, 0, 0), info(4, 1, 1, 1, 1), info(0xFFFFFF, 1, 2, 0, 0), info(3, 2, 1, 0, 0)]
    return w


def test_helpers_on_a_hand_made_list(native_lib):
    w = hand_made(native_lib)
    obj, pas, br, e0, e1 = radar.unpack_wave_info(w["info"])
    assert obj.tolist() == [3, 0xFFFFFF, 4, 0xFFFFFF, 3] and pas.tolist() == [0, 0, 1, 1, 2] and br.tolist() == [0, 0, 1, 2, 1]
    assert e0.tolist() == [1, 0, 1, 0, 0] and e1.tolist() == [0, 0, 1, 0, 0]
    assert radar.unpack_wave_info(np.uint32(0xFFFFFFFF)) == (0xFFFFFF, 15, 3, 1, 1)
    hp = radar.hit_points(w)
    assert hp.dtype == np.float32 and np.array_equal(hp[[0, 2, 4]], np.float32([[2, 0, 0], [2, 1, 0.5], [2, 1, -3.5]])) and np.isnan(hp[[1, 3]]).all()
    assert radar.hit_points(w.reshape(1, 5)).shape == (1, 5, 3)
    assert radar.path_to_wave(w, 4).tolist() == [0, 2, 4] and radar.path_to_wave(w, 1).tolist() == [1] and radar.path_to_wave(w, 3).tolist() == [0, 3]
    for k, chain in ((0, [0]), (1, [0, 2]), (2, [0, 2])):          # echo 2 is wave 2's second (multipath) echo
        c, pts = radar.path_to_echo(w, k)
        assert c.tolist() == chain and pts.shape == (len(chain) + 1, 3) and np.array_equal(pts[0], [0, 0, 0]) and np.array_equal(pts[1:], hp[chain])
    with pytest.raises(IndexError):
        radar.path_to_echo(w, 3)
    with pytest.raises(IndexError):
        radar.path_to_wave(w[:2], 4)          # a truncated list keeps true indices: the helper says so
    loop = w.copy()
    loop["parent"][0] = 4
    with pytest.raises(ValueError):
        radar.path_to_wave(loop, 4)


# ---- the restatement, pinned to the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,rmp", RUNS, ids=IDS)
def test_restatement_equals_the_oracle_log(oracle, case, rmp):
    """waves per pass, and the echo stream echo by echo: count, pass, kind, face, cell, and the strength bit for bit"""
    st, log = logged(oracle, case, rmp)
    assert st["near_threshold"] == 0, case
    for az in AZS:
        waves, pc, ech = reference(oracle, case, rmp, az)
        assert np.array_equal(pc, log["waves"][az, :n_passes(case)]), (case, az, pc, log["waves"][az])
        n = int(log["counts"][az])
        assert len(ech) == n <= log["cells"].shape[1], (case, az, len(ech), n)
        for k, name in (("pass", "passes"), ("kind", "kinds"), ("face", "faces"), ("cell", "cells")):
            bad = np.flatnonzero(ech[k] != log[name][az, :n])
            assert bad.size == 0, (case, az, k, bad[:4], ech[k][bad[:4]], log[name][az, :n][bad[:4]])
        bad = np.flatnonzero(ech["strength"].view(np.uint32) != log["strengths"][az, :n].view(np.uint32))
        assert bad.size == 0, (case, az, "strength", bad[:4], ech["strength"][bad[:4]], log["strengths"][az, :n][bad[:4]])


@pytest.mark.parametrize("case,rmp", RUNS, ids=IDS)
def test_restatement_is_consistent(oracle, case, rmp):
    """the list is what the header defines: passes in sequence, parents in the previous pass, at most one child per branch, no child
    of a miss, echo indices that enumerate the stream"""
    for az in AZS:
        waves, pc, ech = reference(oracle, case, rmp, az)
        check_list(waves, pc, len(ech))
        own = np.flatnonzero(waves["echo"] >= 0)
        assert np.array_equal(ech["wave"][np.r_[True, np.diff(ech["wave"]) != 0]], own), (case, az)


def check_list(waves, pc, n_echoes):
    """the structural rules of one azimuth's list (shared with tests/test_gpu_paths.py)"""
    obj, pas, br, e0, e1 = radar.unpack_wave_info(waves["info"])
    start = np.concatenate([[0], np.cumsum(pc)])
    assert len(waves) == start[-1]
    assert np.array_equal(pas, np.repeat(np.arange(len(pc)), pc))
    first = waves[:pc[0]]
    assert (first["parent"] == -1).all() and (br[:pc[0]] == 0).all() and (first["material"] == 0).all()
    later = np.arange(pc[0], len(waves))
    par = waves["parent"][later]
    assert (par >= start[pas[later] - 1]).all() and (par < start[pas[later]]).all()
    assert np.isin(br[later], (1, 2)).all()
    key = par.astype(np.int64) * 4 + br[later]
    assert (np.diff(key) > 0).all()              # parents rise, reflection before transmission: no parent has two children of one branch
    assert (waves["range"][par] >= 0).all()      # a parent that missed has no child
    miss = waves["range"] < 0
    assert (waves["range"][miss] == -1.0).all() and (waves["face"][miss] == 0xFFFFFFFF).all() and (obj[miss] == 0xFFFFFF).all()
    assert not (e0[miss] | e1[miss]).any() and (waves["face"][~miss] != 0xFFFFFFFF).all()
    has = (e0 | e1) > 0
    assert np.array_equal(has, waves["echo"] >= 0)
    n_own = e0.astype(np.int64) + e1
    assert np.array_equal(waves["echo"][has], (np.cumsum(n_own) - n_own)[has]) and n_own.sum() == n_echoes
    assert not e1[:pc[0]].any()


# ---- the premises of the GPU tests --------------------------------------------------------------------------------------------------
def test_premises_of_the_gpu_tests(oracle):
    """(a) near_threshold == 0 on every case; (b) among the azimuths used, a single pass of more than 256 and one of more than 512
    waves: the gather's sweep loop goes round twice and three times; (c) a wave with both echoes under record_multi_path; (d) a miss;
    (e) every list fits the stride the GPU tests ask for"""
    most, both, miss = 0, 0, 0
    seen = set()
    for case, rmp in RUNS:
        st, log = logged(oracle, case, rmp)
        assert st["near_threshold"] == 0, case                                             # (a)
        w = log["waves"][list(AZS)].astype(np.int64)
        seen |= {1 if 256 < x <= 512 else 2 if x > 512 else 0 for x in w.ravel()}
        assert log["waves"].sum(1).max() <= STRIDE[case], (case, log["waves"].sum(1).max())          # (e)
        for az in AZS:
            waves, _, _ = reference(oracle, case, rmp, az)
            _, _, _, e0, e1 = radar.unpack_wave_info(waves["info"])
            both += int((e0 & e1).sum())
            miss += int((waves["range"] < 0).sum())
            most = max(most, len(waves))
    assert {1, 2} <= seen, seen                                                            # (b)
    assert both > 0 and miss > 0, (both, miss)                                             # (c), (d)


# records per azimuth the GPU tests ask for: above every list of the case (asserted above on the oracle's whole sweep)
STRIDE = {"N": 192, "A": 2048, "B": 3072, "B2": 3072}
