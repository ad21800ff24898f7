"""The frame chain at ragged beam and azimuth counts without a GPU: the cases of tests/test_gpu_ragged.py fixed here -- scene, materials,
config, beams, pose and azimuth window -- together with the premises that file's comparison rests on, checked on the oracle's extended
echo log.  One wave carries 16 rays, a later-pass row is ceil(bound / 16) groups, pass 0 tiles (16 / A) samples x A neighbouring
segments (A = RR_PASS0_AZ) and the later-pass grid comes in chunks of 16 segments: the cases put 1, 2, 3, 5, 7, 15, 17, 31, 33, 63 and
65 beam samples and windows of 1, 2, 3, 15, 16, 17 and 33 azimuths on either side of each of those steps.

The count classes the list attains inside its windows (test_the_list_reaches_every_count_class prints them on failure): later-pass
segments of 1, 2, 3, 15, 16, 17, 31, 32 and 33 waves all occur -- on the oracle, over the 41 windows, later-pass wave counts per
azimuth take 94 different values between 0 and 195; 24 cases hold an azimuth without a live pass-1 wave beside one that has some."""
from collections import namedtuple

import numpy as np
import pytest

import test_stream_host as S
from common import golden_beams, mats_tuple
from radarays_ros_amd import params, scenes

N_CELLS = 256
RESOLUTION = 0.1          # 25.6 m: the far corner of the outer box lies 20.9 m from the sensor
XYZ = (0.1, -0.15, 0.05)
N_BEAMS = (1, 2, 3, 5, 7, 15, 17, 31, 33, 63, 65)
WIDTHS = (1, 2, 3, 15, 16, 17, 33)
N_ANGLES = (400, 37, 17)
CLASSES = (1, 2, 3, 15, 16, 17, 31, 32, 33)

Case = namedtuple("Case", "n_beam n_angles az_begin az_end n_reflections rmp yaw noise")


def _case(n_beam, n_angles, az_begin, az_end, n_reflections, rmp, yaw, noise=0):
    return Case(n_beam, n_angles, az_begin, az_end, n_reflections, rmp, yaw, noise)


# The windows were placed with the oracle over the opening of the scene (below), where hits, misses and azimuths without any live wave lie
# side by side; yaw turns the opening to where the window is wanted (the first and the last azimuths of a sweep).
CASES = [
    _case(1, 400, 17, 20, 4, True, 0.3), _case(1, 37, 1, 18, 2, False, 0.3), _case(1, 17, 0, 16, 3, True, 0.3), _case(1, 400, 1, 34, 1, False, 0.3),
    _case(2, 400, 17, 19, 3, False, 0.3), _case(2, 37, 4, 37, 4, True, 1.1), _case(2, 17, 1, 16, 2, True, 1.1), _case(2, 400, 1, 2, 4, False, 0.3),
    _case(3, 400, 17, 18, 2, True, 0.3), _case(3, 37, 1, 17, 3, False, 0.3), _case(3, 17, 0, 17, 4, True, 0.3), _case(3, 400, 4, 21, 1, True, 0.3),
    _case(5, 400, 7, 22, 4, False, 0.3), _case(5, 37, 1, 3, 1, True, 0.3), _case(5, 17, 14, 17, 3, False, 0.3),
    _case(5, 400, 5, 22, 3, True, 0.3, noise=2),          # the one case with Perlin noise
    _case(7, 400, 1, 34, 2, True, 0.3), _case(7, 37, 1, 2, 3, False, 0.3), _case(7, 17, 2, 4, 4, True, 0.3), _case(7, 400, 384, 400, 4, False, -0.12),
    _case(15, 400, 23, 26, 2, False, 0.3), _case(15, 37, 1, 16, 3, True, 1.1), _case(15, 17, 15, 16, 4, False, 0.3), _case(15, 400, 0, 16, 1, True, 0.05),
    _case(17, 400, 383, 400, 2, True, 0.05), _case(17, 37, 6, 9, 4, False, 1.1), _case(17, 17, 0, 17, 1, False, 0.3), _case(17, 400, 23, 25, 3, True, 0.3),
    _case(31, 400, 1, 2, 3, True, 0.3), _case(31, 37, 0, 33, 2, False, 1.1), _case(31, 17, 1, 16, 1, True, 0.3), _case(31, 400, 11, 26, 4, True, 0.3),
    _case(33, 400, 10, 26, 3, False, 0.3), _case(33, 37, 1, 18, 4, True, 1.1), _case(33, 400, 23, 25, 2, False, 0.3),
    _case(63, 400, 23, 26, 4, False, 0.3), _case(63, 37, 21, 37, 1, False, -0.12), _case(63, 400, 12, 13, 2, True, 0.3),
    _case(65, 400, 1, 34, 3, True, 0.3), _case(65, 17, 1, 3, 2, False, 0.3), _case(65, 400, 0, 15, 4, False, 0.05),
]
IDS = ["b%d-n%d-az%d_%d-p%d%s%s" % (c.n_beam, c.n_angles, c.az_begin, c.az_end, c.n_reflections, "-mp" if c.rmp else "", "-perlin" if c.noise else "")
       for c in CASES]


def width(c):
    return c.az_end - c.az_begin


def _panel(x, y0, y1, h, vbase):
    v = np.float32([[x, y0, -h], [x, y1, -h], [x, y1, h], [x, y0, h]])
    return v, np.uint32([[0, 2, 1], [0, 3, 2]]) + np.uint32(vbase)


_SCENE = []


def scene():
    """two nested boxes whose +x walls have an opening over their full height: object 0, half-size 5 m, penetrable, open for
    y in (-1.2, 0.4); object 1, half-size 12 m, the KAIST wall, open for y in (-3, 0).  From the sensor the inner opening spans
    headings of about -14..+5 degrees and the outer one -14..0: a ray between -14 and 0 leaves the scene (a pass-0 miss), one between
    0 and +5 meets the opaque outer wall first (one child), every other ray the penetrable box (two children).  28 triangles."""
    if not _SCENE:
        vs, fs, ob, vb = [], [], [], 0
        for o, (h, gap) in enumerate(((5.0, (-1.2, 0.4)), (12.0, (-3.0, 0.0)))):
            v, f = scenes._box_tris([-h] * 3, [h] * 3, vbase=vb)
            f = np.array([t for t in f if not all(v[i - vb, 0] == h for i in t)], np.uint32)          # the +x wall goes ...
            vs.append(v); fs.append(f); ob.append(np.full(len(f), o, np.uint32)); vb += 8
            for y0, y1 in ((-h, gap[0]), (gap[1], h)):                                                # ... two panels replace it
                v, f = _panel(h, y0, y1, h, vb)
                vs.append(v); fs.append(f); ob.append(np.full(2, o, np.uint32)); vb += 4
        _SCENE.append({"verts": np.concatenate(vs), "faces": np.concatenate(fs), "face_object_id": np.concatenate(ob),
                       "object_materials": [2, 1], "name": "ragged_boxes"})
    return _SCENE[0]


def materials():
    return params.kaist_materials() + [params.PENETRABLE]


def config(c, n_reflections=None):
    return params.kaist_preset(n_cells=N_CELLS, resolution=RESOLUTION, n_samples=c.n_beam, n_reflections=c.n_reflections if n_reflections is None else n_reflections,
                               ambient_noise=c.noise, signal_denoising=1, signal_denoising_triangular_width=9, record_multi_path=c.rmp)


def beams(c):
    return golden_beams(c.n_beam)


def pose(c):
    return scenes.yaw_pose(XYZ[0], XYZ[1], XYZ[2], c.yaw)


def noise_offsets(c):
    return (np.random.RandomState(c.n_angles).uniform(0, 1, c.n_angles) * 1000.0).astype(np.float32) if c.noise else None


def stride(c):
    """records per azimuth the GPU tests export: every pass' wave bound, twice that with multipath echoes (never exceeded: asserted)"""
    return max(8, c.n_beam * ((1 << c.n_reflections) - 1) * (2 if c.rmp else 1))


_LOGS = {}


def logged(oracle, c, window):
    """(u8, f32, stats, extended echo log) of a case on the oracle -- its whole sweep, or its window alone -- computed once"""
    key = (c, bool(window))
    if key not in _LOGS:
        s = scene()
        sc = oracle.Scene(s["verts"], s["faces"], s["face_object_id"], use_bvh=0)
        log = {"cap": stride(c)}
        b, e = (c.az_begin, c.az_end) if window else (0, c.n_angles)
        u8, f32, st = oracle.simulate(sc, mats_tuple(materials()), s["object_materials"], config(c), beams(c), pose(c), noise_rnd=noise_offsets(c),
                                      az_begin=b, az_end=e, n_angles=c.n_angles, echo_log=log)
        for v in [u8, f32] + list(log.values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)          # shared among the tests that need it, and left unchanged
        _LOGS[key] = (u8, f32, st, log)
    return _LOGS[key]


# ---- the list ---------------------------------------------------------------------------------------------------------------------
def test_every_value_appears_at_least_twice():
    assert 38 <= len(CASES) <= 44 and len(set(CASES)) == len(CASES)
    for values, of in ((N_BEAMS, [c.n_beam for c in CASES]), (WIDTHS, [width(c) for c in CASES]), (N_ANGLES, [c.n_angles for c in CASES]),
                       ((1, 2, 3, 4), [c.n_reflections for c in CASES])):
        assert set(of) == set(values), sorted(set(of))
        for v in values:
            assert of.count(v) >= 2, (v, of.count(v))
    assert all(0 <= c.az_begin < c.az_end <= c.n_angles for c in CASES)
    assert sum(c.az_begin > 0 for c in CASES) >= 2 and sum(c.az_end == c.n_angles for c in CASES) >= 2 and sum(c.az_begin == 0 for c in CASES) >= 2
    assert sum(c.az_begin > 0 and c.az_end < c.n_angles for c in CASES) >= 2
    assert abs(sum(c.rmp for c in CASES) - len(CASES) / 2.0) <= 1.0                     # multipath echoes in half the cases
    assert [c.noise for c in CASES].count(2) == 1 and [c.noise for c in CASES].count(0) == len(CASES) - 1
    s = scene()
    assert len(s["faces"]) == 28 and s["faces"].max() < len(s["verts"]) == 32 and set(s["face_object_id"]) == {0, 1}
    assert materials()[s["object_materials"][0]].velocity > 0 and materials()[s["object_materials"][1]].velocity == 0


# ---- the premises of the GPU tests ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_premises_of_a_case(oracle, c):
    """(a) a pass-0 hit and a miss inside the window; (b) no wave energy within 1e-6 of the pruning threshold anywhere in the sweep,
    where the last ulp of acosf decides a wave's fate; (c) no azimuth's stream is longer than the export stride; (d) the oracle's windowed
    result is its whole sweep cut to the window: image bytes, f32 bits, echo log, and statistics that are the window's sums"""
    u8, f32, st, log = logged(oracle, c, False)
    w8, w32, wst, wlog = logged(oracle, c, True)
    b, e = c.az_begin, c.az_end
    m = S.valid(log)
    assert (m & (log["passes"] == 0))[b:e].any() and wst["hits"] > 0, c                                          # (a)
    assert wst["wave_passes"] > wst["hits"], (c, wst)
    assert st["near_threshold"] == 0 and wst["near_threshold"] == 0, (c, st)                                     # (b)
    assert log["counts"].max() <= stride(c) and (log["waves"][:, 0] == c.n_beam).all(), c                         # (c)
    assert np.array_equal(w8[:, b:e], u8[:, b:e]) and np.array_equal(w32[:, b:e].view(np.uint32), f32[:, b:e].view(np.uint32)), c          # (d)
    out = np.ones(c.n_angles, bool)
    out[b:e] = False
    assert not w8[:, out].any() and not w32[:, out].any() and not wlog["counts"][out].any() and not wlog["waves"][out].any(), c
    for k in ("cells", "faces", "passes", "kinds", "frac", "counts", "waves"):
        assert np.array_equal(wlog[k][b:e], log[k][b:e]), (c, k)
    assert np.array_equal(wlog["strengths"][b:e].view(np.uint32), log["strengths"][b:e].view(np.uint32)), c
    assert wst["wave_passes"] == log["waves"][b:e].sum() and wst["signals"] == log["counts"][b:e].sum(), (c, wst)
    assert st["wave_passes"] == log["waves"].sum() and st["signals"] == log["counts"].sum(), (c, st)
    assert (m & (log["kinds"] == 1)).any() == (c.rmp and c.n_reflections > 1) or not c.rmp, c
    if c.noise:
        quiet = oracle.simulate(oracle.Scene(scene()["verts"], scene()["faces"], scene()["face_object_id"], use_bvh=0), mats_tuple(materials()),
                                scene()["object_materials"], config(c._replace(noise=0)), beams(c), pose(c), n_angles=c.n_angles, want_f32=False)[0]
        assert not np.array_equal(quiet[:, b:e], u8[:, b:e])                                                    # the noise shows


def later_counts(oracle, c):
    """[width][n_reflections - 1] waves per azimuth of the window at the start of each later pass"""
    return logged(oracle, c, False)[3]["waves"][c.az_begin:c.az_end, 1:].astype(np.int64)


def test_the_list_reaches_every_count_class(oracle):
    """over the whole list, inside the windows, the later-pass wave counts per azimuth take each of 1..3, 15..17 and 31..33"""
    seen = set()
    for c in CASES:
        seen |= set(int(x) for x in later_counts(oracle, c).ravel())
    assert set(CLASSES) <= seen, ("missing", sorted(set(CLASSES) - seen), "attained", sorted(seen))
    assert len(seen) >= 40 and max(seen) > 8 * 16, sorted(seen)                       # ... and rows of one group and of more than eight


def test_some_azimuth_has_no_live_wave_beside_one_that_has(oracle):
    """pass 1 of an azimuth inside a window starts with no wave at all (every beam sample left through the opening) while an azimuth
    next to it, inside the window too, has some: a segment row of the later-pass grids that exits at once between rows that work"""
    found = []
    for c, name in zip(CASES, IDS):
        if c.n_reflections > 1 and width(c) >= 2:
            n1 = later_counts(oracle, c)[:, 0]
            if ((n1[1:] == 0) & (n1[:-1] > 0)).any() or ((n1[:-1] == 0) & (n1[1:] > 0)).any():
                found.append(name)
    assert len(found) >= 3, found
