"""Doppler without a GPU: the entry points of include/radarays_mi355.h ("Doppler"), the numpy restatement of the definition
(tests/doppler_ref.py) against closed forms on hand-made chains, and the premises tests/test_gpu_doppler.py rests on, proven on the
oracle-built lists of tests/test_paths_host.py alone (its cases N, A, B, B2 at its azimuths AZS).

The twists give object 1 both a linear and an angular velocity; GAIN moves echoes by a few bins, GAIN_EDGE (the other chirp direction,
twelve times as strong) pushes echoes over both image edges.  Both were chosen so that on case N no r' / resolution of the oracle-built
lists lies within 1e-3 of an integer (test_premises_of_the_gpu_tests): the cap that keeps the bit-exact cell checks of the definition
test honest.  The lists of A, B and B2 hold ten thousand echoes and more; no gain keeps all of them that far from an integer, so where
the GPU tests use B2 (the one case with echoes pushed below range zero) the cells follow from the bit-equal v_r asserted beside them."""
import os

import numpy as np
import pytest

import doppler_ref as D
import paths_ref as R
import test_paths_host as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
TWISTS = np.float32([[0, 0, 0, 0, 0, 0], [6.0, -3.0, 0.5, 0.0, 0.0, 0.4]])      # object 1: V and Omega both nonzero
V_S = np.float32([4.0, 2.0, 0.0])
GAIN = 0.05
GAIN_EDGE = -0.61


# ---- the interface ------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound(native_lib):
    header = open(os.path.join(ROOT, "include", "radarays_mi355.h")).read()
    assert "#define RR_ABI_VERSION 7" in header and native_lib.lib().rr_abi_version() == 7          # purely additive
    assert "UNPINNED" in header.split("---- Doppler")[1].split("int rr_simulate_batch_doppler_device(")[0]
    for m in ("set_object_twists", "simulate_batch_doppler_device", "simulate_doppler"):
        assert callable(getattr(native_lib.Context, m))
    from radarays_ros_amd import radar
    assert callable(radar.RadarHIP.simulate_doppler)
    assert "simulateDoppler" in open(os.path.join(ROOT, "include", "radarays_ros_amd", "RadarHIP.hpp")).read()


def test_calls_without_a_context_are_refused(native_lib):
    Lb = native_lib.lib()
    assert Lb.rr_set_object_twists(None, None, 0) == -1
    assert Lb.rr_simulate_batch_doppler_device(None, None, 1, None, 0.0, None, None, 0, None, None, None, None) == -1
    assert Lb.rr_simulate_doppler(None, None, None, 0.0, None, None, None, 0, None, None, None) == -1


# ---- the restatement on hand-made chains: closed forms --------------------------------------------------------------------------------
def wave(native_lib, o, d, rng, obj, pas, parent, echo, e0=1, e1=0, time=0.0):
    w = np.zeros(1, native_lib.WAVE_DTYPE)
    w["o"], w["d"], w["range"], w["parent"], w["echo"], w["time"] = [o], [d], rng, parent, echo, time
    w["info"] = (obj & 0xFFFFFF) | pas << 24 | e0 << 30 | e1 << 31
    return w


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v)).astype(F)


def test_static_scene_and_moving_sensor(native_lib):
    """v_r = -(v_s . u_0) = -u_0.x for v_s = (1, 0, 0), whatever the beam"""
    dirs = [unit(d) for d in ([1, 0, 0], [0, 1, 0], [1, 2, 3], [-3, 1, 0.5])]
    w = np.concatenate([wave(native_lib, [0, 0, 0], d, 5.0, 0, 0, -1, k) for k, d in enumerate(dirs)])
    vr, cell, _ = D.doppler(w, w, len(dirs), np.zeros((1, 6), F), [1, 0, 0], 0.0, 0.05)
    assert np.array_equal(vr, np.float32([-d[0] for d in dirs])) and vr.dtype == F


def test_wall_moving_along_its_own_plane(native_lib):
    """a wall x = 4 seen at normal incidence, sliding along y and z: the range does not change"""
    w = wave(native_lib, [0, 0, 0], [1, 0, 0], 4.0, 0, 0, -1, 0)
    vr, _, _ = D.doppler(w, w, 1, np.float32([[0, 2.5, -1.5, 0, 0, 0]]), [0, 0, 0], 0.0, 0.05)
    assert vr[0] == 0.0


def test_wall_receding_along_its_normal(native_lib):
    w = wave(native_lib, [0, 0, 0], [1, 0, 0], 4.0, 0, 0, -1, 0)
    for s in (0.75, -3.0, 12.5):
        vr, cell, sd = D.doppler(w, w, 1, np.float32([[s, 0, 0, 0, 0, 0]]), [0, 0, 0], 0.5, 0.05)
        assert vr[0] == F(s)
        assert cell[0] == int(float(F(sd[0] + F(0.5) * F(s))) / 0.05)
    # a rotation about the map origin moves the hit point (4, 0, 0) along y: still nothing along the beam
    assert D.doppler(w, w, 1, np.float32([[0, 0, 0, 0, 0, 0.7]]), [0, 0, 0], 0.0, 0.05)[0][0] == 0.0


def test_two_bounce_ghost_by_hand(native_lib):
    """beam along +x hits a moving mirror (object 1) at p_0 = (3, 0, 0) and leaves along +y to a static wall (object 0) at p_1 =
    (3, 2, 0); sensor static: dL/dt = v_0 . (u_0 - u_1) + v_1 . u_1 with v_1 = 0, written out in f32"""
    tw = np.float32([[0, 0, 0, 0, 0, 0], [1.25, -0.5, 0.25, 0.1, -0.2, 0.3]])
    w = np.concatenate([wave(native_lib, [0, 0, 0], [1, 0, 0], 3.0, 1, 0, -1, -1, e0=0), wave(native_lib, [3, 0, 0], [0, 1, 0], 2.0, 0, 1, 0, 0, time=10.0)])
    vr, _, _ = D.doppler(w, w, 1, tw, [0, 0, 0], 0.0, 0.05)
    V, Om, p0 = tw[1, :3], tw[1, 3:], np.float32([3, 0, 0])
    v0 = (V[0] + (Om[1] * p0[2] - Om[2] * p0[1]), V[1] + (Om[2] * p0[0] - Om[0] * p0[2]), V[2] + (Om[0] * p0[1] - Om[1] * p0[0]))
    du = (F(1) - F(0), F(0) - F(1), F(0) - F(0))
    acc = F(-F(0.0)) + (v0[0] * du[0] + v0[1] * du[1] + v0[2] * du[2])
    want = acc + (F(0) * F(0) + F(0) * F(1) + F(0) * F(0))
    assert vr[0] == want and vr.dtype == F and want != 0
    # the same ghost as a multipath echo: half of the way out plus the way straight home, e = (3, 2, 0) / |.|
    w["info"][1] |= np.uint32(1 << 31)
    vr2, _, _ = D.doppler(w, w, 2, tw, [0, 0, 0], 0.0, 0.05)
    assert vr2[0] == want and vr2[1] == F(0.5) * (want + F(0.0))


# ---- gain = 0 is the chain's cell, on the oracle-built lists ------------------------------------------------------------------------
def lists(oracle, case, rmp, az):
    wm, _, ech = H.reference(oracle, case, rmp, az, True)
    ws, _, _ = H.reference(oracle, case, rmp, az, False)
    return wm, ws, ech


@pytest.mark.parametrize("case,rmp", H.RUNS, ids=H.IDS)
def test_gain_zero_returns_the_chain_cells(oracle, case, rmp):
    res = H.config(case, rmp).resolution
    for az in H.AZS:
        wm, ws, ech = lists(oracle, case, rmp, az)
        for tw, vs, gain in ((TWISTS, V_S, 0.0), (np.zeros((2, 6), F), np.zeros(3, F), GAIN)):
            vr, cell, _ = D.doppler(wm, ws, len(ech), tw, vs, gain, res)
            assert np.array_equal(cell, ech["cell"]), (case, az, np.flatnonzero(cell != ech["cell"])[:4])
            assert gain == 0.0 or not vr.any()


# ---- the premises of the GPU tests --------------------------------------------------------------------------------------------------
def test_premises_of_the_gpu_tests(oracle):
    """(a) with TWISTS, V_S and GAIN at least one echo of every case moves by at least one bin; (b) at least one multipath echo moves;
    (c) with GAIN_EDGE an echo inside the image leaves it over the far edge, and one falls below range zero and is dropped (cell' = -1);
    (d) on case N, under GAIN and under GAIN_EDGE, no r' / resolution lies within 1e-3 of an integer"""
    near = far = 0
    for case, rmp in H.RUNS:
        cfg = H.config(case, rmp)
        moved = mp = 0
        for gain in (GAIN, GAIN_EDGE):
            for az in H.AZS:
                wm, ws, ech = lists(oracle, case, rmp, az)
                vr, cell, sd = D.doppler(wm, ws, len(ech), TWISTS, V_S, gain, cfg.resolution)
                c0 = ech["cell"].astype(np.int64)
                if gain == GAIN:
                    moved += int((np.abs(cell - c0) >= 1).sum())
                    mp += int(((ech["kind"] == 1) & (cell != c0)).sum())
                else:
                    near += int((cell == -1).sum())
                    far += int(((c0 < cfg.n_cells) & (cell >= cfg.n_cells)).sum())
                if case == "N":
                    q = (sd + F(gain) * vr).astype(np.float64) / cfg.resolution
                    assert np.abs(q - np.round(q)).min() >= 1e-3, (case, rmp, gain, az)          # (d)
        assert moved > 0, case                                                                     # (a)
        assert mp > 0 or not rmp, case                                                             # (b)
    assert near > 0 and far > 0, (near, far)                                                       # (c)
