"""The echo stream at multi-batch sizes without a GPU: the cases of tests/test_gpu_stream.py fixed here -- scene, materials, config,
beams and pose -- together with the premises that file's comparison rests on, checked on the oracle's extended echo log
(oracle.simulate(echo_log=...): faces, passes, kinds, frac, waves).  The kernels that decide which echoes exist and in what order
(k_trace, k_shade, k_scan, k_echo_gather) walk a segment's waves 256 at a time and k_column its echoes 1,024 at a time: every case
has passes of 257..512 and of more than 512 waves and azimuths of more than 1,024 echoes."""
import numpy as np
import pytest

import test_labels_host as L
from common import golden_beams, mats_tuple
from radarays_ros_amd import params, scenes

N_ANGLES = 400
BATCH = 256                    # waves per sweep of k_scan / k_echo_gather / k_shade
SIG_CHUNK = 1024               # RR_SIG_CHUNK: echoes per staging round of k_column

# A later-pass echo is MARGINAL where its f64 fractional position inside its range bin lies within DELTA of a bin boundary: there the
# one-ulp difference between the GPU's libm and the host's in the chain behind the echo's time may move it to the neighbouring bin,
# and only there.  Measured on the MI355X against the oracle's log: of 2.7 million later-pass echoes over the six
# runs ONE lands in the neighbouring bin -- case B2, azimuth 181, a pass-3 path echo 298 m out, oracle cell 5012 at frac
# 0.000460123199, GPU cell 5011 (the same echo in the path and the multipath run; far outside the 1,024-cell image).  DELTA is eight
# times the largest margin seen, below the 5e-3 beyond which a flip is not rounding.  Premise (e) below keeps the allowance from
# hiding anything: at most 1 % of the later-pass echoes are marginal (a flat fractional position gives 2 * DELTA = 0.74 %).
FLIP_MARGIN = 0.000460123199
DELTA = 8 * FLIP_MARGIN
assert DELTA <= 5e-3

_SCENES = {}


def scene(case):
    key = "A" if case == "A" else "B"
    if key not in _SCENES:
        _SCENES[key] = L.scene() if key == "A" else scenes.heightfield_room(40, n_buildings=30)
    return _SCENES[key]


def materials(case):
    return L.materials() if case == "A" else params.kaist_materials() + [params.PENETRABLE]


def n_samples(case):
    return 300 if case == "A" else 200


def n_reflections(case):
    return 3 if case == "A" else 4


def config(case, rmp=False, passes=None):
    """case A: the nested boxes of tests/test_labels_host.py with 300 beam samples; cases B, B2: the KAIST preset on the terrain"""
    p = n_reflections(case) if passes is None else passes
    if case == "A":
        return params.kaist_preset(n_cells=512, resolution=0.05, n_samples=300, n_reflections=p, ambient_noise=0, signal_denoising=1,
                                   signal_denoising_triangular_width=9, record_multi_path=rmp)
    return params.kaist_preset(n_reflections=p, n_samples=200, ambient_noise=0, n_cells=1024, record_multi_path=rmp)


def beams(case):
    return golden_beams(n_samples(case))


def pose(case):
    """B: the scene's default pose, in the open.  B2: one metre above the ground in the 2.5 m gap between two buildings (footprints
    y = 59.6..71.6 and y = 74.1..87.9 around x = -50): nearly every wave meets a penetrable wall, the later passes hold a third more
    waves than at B -- the situation of tests/test_gpu_round5.py::test_tight_trace_rows_follow_the_history_and_never_change_an_image"""
    if case == "A":
        return L.POSE3[1]
    if case == "B":
        return scenes.default_pose(scene("B")["name"])
    return scenes.yaw_pose(-50.0, 72.8, float(scenes.ground_height(-50.0, 72.8)) + 1.0, 0.3)


def wave_capacity(case):
    """the lane's wave queue per azimuth and pass with max_waves_per_azimuth left at 0 (include/radarays_mi355.h)"""
    return min(n_samples(case) << (n_reflections(case) - 1), 65536)


def tight_row(h):
    """rays in a later-pass trace row after a batch whose longest segment held h waves (tight trace rows)"""
    return (((h + h // 16 + 32 + 15) // 16) | 1) * 16


CASES = ("A", "B", "B2")
# exported records per azimuth the GPU tests ask for: above every count of the case (asserted below), below the log's cap
STRIDE = {"A": 1536, "B": 2432, "B2": 2688}
CAP = 4096

_LOGS = {}


def logged(oracle, case, rmp, passes=None):
    """the oracle's image, stats and extended echo log of one case, computed once"""
    key = (case, bool(rmp), n_reflections(case) if passes is None else passes)
    if key not in _LOGS:
        s = scene(case)
        sc = oracle.Scene(s["verts"], s["faces"], s["face_object_id"], use_bvh=0 if case == "A" else 1)
        log = {}
        u8, _, st = oracle.simulate(sc, mats_tuple(materials(case)), s["object_materials"], config(case, rmp, key[2]), beams(case), pose(case),
                                    echo_log=log, want_f32=False)
        for v in log.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)          # shared among the tests that need it, and left unchanged
        _LOGS[key] = (u8, st, log)
    return _LOGS[key]


def valid(log):
    """[n_angles][cap] True on the logged echoes"""
    return np.arange(log["cells"].shape[1])[None, :] < log["counts"][:, None]


def margin(log):
    return np.minimum(log["frac"], 1.0 - log["frac"])


# ---- the log itself -----------------------------------------------------------------------------------------------------------------
def test_extended_log_keeps_the_old_keys_and_changes_no_image(oracle):
    s = scene("A")
    sc = oracle.Scene(s["verts"], s["faces"], s["face_object_id"], use_bvh=0)
    args = (sc, mats_tuple(materials("A")), s["object_materials"], config("A", True), beams("A"), pose("A"))
    u8, f32, st = oracle.simulate(*args)
    log = {"cap": 1000}
    v8, w32, st2 = oracle.simulate(*args, echo_log=log)
    assert np.array_equal(u8, v8) and np.array_equal(f32.view(np.uint32), w32.view(np.uint32))
    assert {k: v for k, v in st.items() if k != "seconds"} == {k: v for k, v in st2.items() if k != "seconds"}
    assert set(log) == {"cap", "cells", "strengths", "counts", "faces", "passes", "kinds", "frac", "waves"} and log["cap"] == 1000
    want = {"cells": np.int32, "strengths": np.float32, "faces": np.uint32, "passes": np.uint8, "kinds": np.uint8, "frac": np.float64}
    for k, dt in want.items():
        assert log[k].dtype == dt and log[k].shape == (N_ANGLES, 1000), k
    assert log["counts"].dtype == np.uint32 and log["counts"].shape == (N_ANGLES,)
    assert log["waves"].dtype == np.uint32 and log["waves"].shape == (N_ANGLES, 3)
    _, _, full = logged(oracle, "A", True)
    assert full["cells"].shape == (N_ANGLES, CAP)                         # the default cap
    assert np.array_equal(log["counts"], full["counts"]) and log["counts"].max() > 1000          # true counts, the first `cap` echoes
    for k in want:
        assert np.array_equal(log[k], full[k][:, :1000]), k
    assert np.array_equal(log["waves"], full["waves"])
    # the plain hook alone still works, and the extended one reads nothing once the plain one is cleared
    Lb = oracle.lib()
    cells, strs, cnt = np.full((N_ANGLES, 8), -1, np.int32), np.zeros((N_ANGLES, 8), np.float32), np.zeros(N_ANGLES, np.uint32)
    Lb.orc_set_echo_log(cells.ctypes.data, strs.ctypes.data, cnt.ctypes.data, 8)
    try:
        x8, _, _ = oracle.simulate(*args, want_f32=False)
    finally:
        Lb.orc_set_echo_log(None, None, None, 0)
    assert np.array_equal(x8, u8) and np.array_equal(cnt, full["counts"]) and np.array_equal(cells, full["cells"][:, :8])


@pytest.mark.parametrize("rmp", [False, True], ids=["path", "multipath"])
@pytest.mark.parametrize("case", CASES)
def test_log_is_consistent_with_itself(oracle, case, rmp):
    """passes never fall along a stream; a pass holds at most one path echo per wave and at most one multipath echo per path echo
    slot; pass 0 and a run with the switch off hold no multipath echo; frac is the fractional part of a position whose integer part
    is the cell; in case A the face of a pass-0 echo lies on the box its range band names"""
    _, st, log = logged(oracle, case, rmp)
    m, P = valid(log), n_reflections(case)
    assert log["waves"].sum() == st["wave_passes"] and log["counts"].sum() == st["signals"], case
    assert (log["waves"][:, 0] == n_samples(case)).all()
    pas = np.where(m, log["passes"], P - 1)
    assert (np.diff(pas.astype(int), axis=1) >= 0).all() and pas.max() == P - 1, case
    for p in range(P):
        of_pass = m & (log["passes"] == p)
        assert ((of_pass & (log["kinds"] == 0)).sum(1) <= log["waves"][:, p]).all(), (case, p)
        assert ((of_pass & (log["kinds"] == 1)).sum(1) <= log["waves"][:, p]).all(), (case, p)
    assert not (m & (log["kinds"] == 1) & (log["passes"] == 0)).any() and (rmp or not (m & (log["kinds"] == 1)).any())
    assert (log["kinds"][m] <= 1).all() and (log["faces"][m] < len(scene(case)["faces"])).all()
    fr = log["frac"][m]
    assert (fr >= 0).all() and (fr < 1).all() and (log["cells"][m] >= 0).all()
    if case == "A":
        p0 = m & (log["passes"] == 0)
        near = (log["cells"] >= L.NEAR_BAND[0]) & (log["cells"] <= L.NEAR_BAND[1])
        obj = scene("A")["face_object_id"][np.where(m, log["faces"], 0)]
        assert np.array_equal(near[p0], obj[p0] == 0)


# ---- the figures the cases were chosen by ------------------------------------------------------------------------------------------
def test_case_a_figures(oracle):
    (_, st0, off), (_, st1, on) = logged(oracle, "A", False), logged(oracle, "A", True)
    assert st0["wave_passes"] == st1["wave_passes"] == 607658 and round(607658 / N_ANGLES) == 1519
    assert (off["counts"].min(), off["counts"].max()) == (897, 900)
    assert (on["counts"].min(), on["counts"].max()) == (910, 1500)
    assert (on["counts"] > SIG_CHUNK).sum() == 376


def test_case_b_figures(oracle):
    assert len(scene("B")["faces"]) == 2 * 40 * 40 + 12 + 12 * 30
    (_, st0, off), (_, st1, on) = logged(oracle, "B", False), logged(oracle, "B", True)
    assert st0["wave_passes"] == st1["wave_passes"] == 446821
    assert (off["counts"].min(), off["counts"].max()) == (800, 1331)
    assert (on["counts"].min(), on["counts"].max()) == (1005, 2343)
    assert (on["counts"] > SIG_CHUNK).sum() == 397 and (on["counts"] > 2 * SIG_CHUNK).sum() == 22


def test_second_pose_of_case_b_needs_longer_rows_than_the_first(oracle):
    """after a batch at pose B the later-pass rows are sized by B's longest segment; some pass of B2 has a segment beyond that row
    and inside the full one: the repair launch has work (tests/test_gpu_stream.py asserts repaired groups > 0)"""
    first, second = logged(oracle, "B", True)[2]["waves"].max(0), logged(oracle, "B2", True)[2]["waves"].max(0)
    over = [p for p in range(1, 4) if tight_row(int(first[p])) < second[p] and tight_row(int(first[p])) < min(200 << p, wave_capacity("B"))]
    assert over, (first, second)
    assert (logged(oracle, "B2", True)[2]["counts"] > 2 * SIG_CHUNK).sum() > 100


# ---- the premises of the GPU tests ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rmp", [False, True], ids=["path", "multipath"])
@pytest.mark.parametrize("case", CASES)
def test_premises_of_the_gpu_tests(oracle, case, rmp):
    """(a) no wave energy within 1e-6 of the pruning threshold; (b) a pass of 257..512 waves and one of more than 512: second and third
    sweeps of the 256-wave loops, none beyond the lane's capacity; (c) an azimuth of more than 1,024 echoes (with multipath: case A's
    path streams stay at 900, B's do cross), all below the export stride and the log's cap; (d) an azimuth whose next pass holds more
    waves than this one: some parent has both a reflection and a refraction child; multipath echoes exist when switched on;
    (e) at most 1 % of the later-pass echoes are marginal; (f) the stream at n_reflections = P begins with the stream at P - 1"""
    what = "%s/%s" % (case, "multipath" if rmp else "path")
    P = n_reflections(case)
    _, st, log = logged(oracle, case, rmp)
    _, st_lo, lo = logged(oracle, case, rmp, P - 1)
    assert st["near_threshold"] == 0 and st_lo["near_threshold"] == 0, what                 # (a)
    w = log["waves"].astype(np.int64)
    assert ((w > BATCH) & (w <= 2 * BATCH)).any(), (what, w.max(0))                        # (b)
    assert (w > 2 * BATCH).any(), (what, w.max(0))
    assert w.max() <= wave_capacity(case), (what, w.max(), wave_capacity(case))
    n = log["counts"].astype(np.int64)                                                     # (c)
    if rmp or case != "A":
        assert (n > SIG_CHUNK).any(), (what, n.max())
    else:
        assert n.max() > 3 * BATCH, (what, n.max())
    assert n.max() <= STRIDE[case] < CAP, (what, n.max())
    assert (w[:, 1:] > w[:, :-1]).any(), what                                              # (d)
    m = valid(log)
    assert (m & (log["kinds"] == 1)).any() == rmp, what
    later = m & (log["passes"] > 0)                                                        # (e)
    share = float((margin(log)[later] < DELTA).mean())
    assert later.sum() > 100000 and share <= 0.01, (what, share)
    assert (lo["counts"] <= log["counts"]).all() and (lo["counts"] < log["counts"]).any(), what          # (f)
    ml = valid(lo)
    for k in ("cells", "faces", "passes", "kinds", "frac"):
        assert np.array_equal(lo[k][ml], log[k][ml]), (what, k)
    assert np.array_equal(lo["strengths"][ml].view(np.uint32), log["strengths"][ml].view(np.uint32)), what
    assert np.array_equal(lo["waves"], log["waves"][:, :P - 1]), what
