"""The beam model on the GPU (rr_scan_profile, rr_cast_map, rr_score_beams) against tests/cast_ref.py, byte for byte and on guarded buffers: the
ranges of every map, grid, saturation and bin step of cast_ref at an azimuth count of two ragged lane tiles, and of a smaller set at every other
azimuth count; the records at the edges of a wave's and a workgroup's hypothesis tile; the profile; the host forms and the refusals; a score
call beside a batch in flight; the closed loop on the GPU's own images; the façade."""
import ctypes as C
import math

import numpy as np
import pytest

import cast_ref as R
import field_ref as F
import icp_ref
import occupancy_ref as O
from common import golden_beams
from radarays_ros_amd import native, params, radar

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
GUARD = 0xA5


def context(n_angles, resolution, scroll=0):
    c = native.Context(0)
    c.set_config(params.kaist_preset(n_cells=R.N_CELLS, resolution=resolution, scroll_image=scroll), n_angles)
    return c


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)


def guarded(n_bytes):
    return torch.full((n_bytes + 64,), GUARD, dtype=torch.uint8, device=DEV)


def payload(t, n_bytes):
    raw = t.cpu().numpy()
    assert np.all(raw[n_bytes:] == GUARD)                             # nothing behind the buffer
    return raw[:n_bytes].copy()


def run_cast(c, states, d_dirs, n_angles, d_field, cfg, beam, stream=None):
    """the device form on a guarded buffer -> uint16 [n][n_angles]"""
    n = len(states)
    d_st, d_out = dev(states), guarded(2 * n * n_angles)
    torch.cuda.synchronize()
    c.cast_map_device(d_st.data_ptr(), n, d_dirs.data_ptr(), d_field.data_ptr(), cfg, beam, d_out.data_ptr(), stream)
    torch.cuda.synchronize()
    return payload(d_out, 2 * n * n_angles).view(np.uint16).reshape(n, n_angles)


def run_score(c, first, states, d_dirs, d_field, cfg, beam, stream=None):
    """the device form on a guarded buffer -> BEAM_DTYPE [n]"""
    n = len(states)
    d_first, d_st, d_out = dev(first), dev(states), guarded(32 * n)
    torch.cuda.synchronize()
    c.score_beams_device(d_first.data_ptr(), d_st.data_ptr(), n, d_dirs.data_ptr(), d_field.data_ptr(), cfg, beam, d_out.data_ptr(), stream)
    torch.cuda.synchronize()
    return payload(d_out, 32 * n).view(native.BEAM_DTYPE)


# ---- 1. ranges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(R.GRIDS)))
def test_ranges_of_every_map_saturation_and_bin_step(k):
    """cast_ref.full_cases: 65 azimuths, one full lane tile and one lane of the next"""
    A = R.FULL_ANGLES
    c = context(A, R.GRIDS[k][3])
    names, sts, cases = R.full_cases(k)
    d_dirs = dev(cases[0]["dirs"])
    for case in cases:
        want = R.case_brute(case)                                     # once for the whole grid
        assert (want < R.N_CELLS).any() and (want == R.N_CELLS).any()
        at = 0
        for i, (name, md) in enumerate(names):
            got = run_cast(c, sts[i], d_dirs, A, dev(case["fields"][i]), R.grid_cfg(k, md), case["beam"])
            assert np.array_equal(got, want[at:at + len(sts[i])]), (k, name, md, case["step"])
            at += len(sts[i])


@pytest.mark.parametrize("A", [a for a in R.ANGLES if a != R.FULL_ANGLES])
def test_ranges_at_every_azimuth_count(A):
    """cast_ref.azimuth_cases"""
    c = context(A, R.GRIDS[R.AZIMUTH_GRID][3])
    n = 0
    for case in R.azimuth_cases(A):
        got = run_cast(c, case["states"], dev(case["dirs"]), A, dev(case["field"]), case["cfg"], case["beam"])
        assert np.array_equal(got, R.case_brute(case)), case["label"]
        n += 1
    assert n == len(R.AZIMUTH_MAPS) * len(R.BIN_STEPS) * len(R.WINDOWS)


# ---- 2. records -----------------------------------------------------------------------------------------------------------------------------
def test_records_at_every_hypothesis_count_and_profile():
    """cast_ref.records_case"""
    A, tol = R.RECORD_ANGLES, R.RECORD_TOL
    _, per_wave, per_group = native.cast_tile_sizes()
    case = R.records_case(per_wave, per_group)
    cfg, fld, dirs, pool, beam, res, rs, counts = (case[k] for k in ("cfg", "field", "dirs", "states", "beam", "res", "rs", "counts"))
    c = context(A, res)
    d_dirs, d_fld = dev(dirs), dev(fld)
    e = R.brute(pool[:1], dirs, fld, cfg, beam, res)[0].astype(np.int64)
    assert (e < 240).all() and (e >= 10 + tol + 1).all()             # the centre sees the ring on every azimuth
    at_edges = np.clip(e + np.resize([-tol - 1, -tol, 0, tol, tol + 1], A), 0, R.N_CELLS)
    profiles = {"none": np.full(A, R.N_CELLS), "below": np.full(A, 9), "edges": at_edges, "mixed": np.where(np.arange(A) % 3 == 0, R.N_CELLS, at_edges),
                "random": rs.randint(0, R.N_CELLS + 1, A)}
    for name, prof in profiles.items():
        first = prof.astype(np.uint16)
        for n in counts:
            got = run_score(c, first, pool[:n], d_dirs, d_fld, cfg, beam)
            want = R.score(first, pool[:n], dirs, fld, cfg, beam, res)
            assert got.tobytes() == want.tobytes(), (name, n)
        full = R.score(first, pool[:257], dirs, fld, cfg, beam, res)
        assert np.all(full["n_agree"] + full["n_short"] + full["n_through"] + full["n_open"] + full["n_none"] == full["n_cast"])
        if name == "below":
            assert not full["n_cast"].any() and not full["sum_abs"].any()
        if name == "none":
            assert np.all(full["n_cast"] == A) and not full["n_agree"].any() and full["n_through"][0] == A
        if name == "edges":
            assert full["n_agree"][0] == sum(1 for j in range(A) if j % 5 in (1, 2, 3)) and full["n_short"][0] > 0 and full["n_through"][0] > 0
    empty = case["empty_beam"]
    got = run_score(c, profiles["random"].astype(np.uint16), pool[:per_group + 1], d_dirs, d_fld, cfg, empty)
    assert got.tobytes() == R.score(profiles["random"].astype(np.uint16), pool[:per_group + 1], dirs, fld, cfg, empty, res).tobytes()
    assert not (got["n_agree"].any() or got["n_short"].any() or got["n_through"].any() or got["n_open"].any() or got["sum_abs"].any())


# ---- 3. profile -----------------------------------------------------------------------------------------------------------------------------
def some_clouds(rs, n, A, n_cells):
    """n clouds sorted by column, then bin, with empty columns -> (clouds, offsets uint32 [n][A + 1])"""
    clouds, offs = [], np.zeros((n, A + 1), np.uint32)
    for f in range(n):
        per = np.where(rs.random_sample(A) < 0.3, 0, rs.randint(1, 4, A))
        if f == 1:
            per[:] = 0                                                # an empty scan
        p = np.zeros(int(per.sum()), native.POINT_DTYPE)
        at = 0
        for col in range(A):
            p["column"][at:at + per[col]] = col
            p["bin"][at:at + per[col]] = np.sort(rs.choice(n_cells, per[col], replace=False))
            at += per[col]
        p["x"], p["intensity"] = rs.uniform(-5, 5, len(p)), 7.0
        clouds.append(p)
        offs[f, 1:] = np.cumsum(per)
    return clouds, offs


@pytest.mark.parametrize("scroll", [0, 5])
def test_profile_matches_the_restatement(scroll):
    A, n = 65, 3
    c = context(A, 0.1, scroll)
    clouds, offs = some_clouds(np.random.RandomState(3 + scroll), n, A, R.N_CELLS)
    longest = max(len(p) for p in clouds)
    assert np.array_equal(c.scan_profile(clouds, offs), R.profile(clouds, offs, R.N_CELLS, A, scroll))          # the host form
    for mp in (longest, longest // 2, 1, 0):
        buf = np.zeros((n, max(mp, 1)), native.POINT_DTYPE)
        for f, p in enumerate(clouds):
            buf[f, :min(len(p), mp)] = p[:mp]
        d_pts, d_offs, d_out = dev(buf), dev(offs), guarded(2 * n * A)
        torch.cuda.synchronize()
        c.scan_profile_device(d_pts.data_ptr() if mp else None, d_offs.data_ptr(), n, mp, d_out.data_ptr())
        c.synchronize()
        got = payload(d_out, 2 * n * A).view(np.uint16).reshape(n, A)
        want = R.profile(clouds, offs, R.N_CELLS, A, scroll, max_points=mp)
        assert np.array_equal(got, want), (scroll, mp)
        if mp == 0:
            assert np.all(got == R.N_CELLS)
        if mp == longest // 2:
            assert (got != R.profile(clouds, offs, R.N_CELLS, A, scroll)).any()       # the cut shows


# ---- 4. host forms, refusals, two streams -----------------------------------------------------------------------------------------------------
def test_the_host_forms_equal_the_device_forms():
    """cast_ref.small_case; and the grid's gate is ignored: a value the likelihood field would refuse changes nothing"""
    A = R.FULL_ANGLES
    case = R.small_case(A)
    cfg, fld, dirs, sts, first, res, beam = (case[k] for k in ("cfg", "field", "dirs", "states", "first", "res", "beam"))
    c = context(A, res)
    d_dirs, d_fld = dev(dirs), dev(fld)
    ranges = run_cast(c, sts, d_dirs, A, d_fld, cfg, beam)
    assert np.array_equal(ranges, R.case_brute(case))
    assert np.array_equal(c.cast_map(sts, dirs, fld, cfg, beam), ranges)
    recs = run_score(c, first, sts, d_dirs, d_fld, cfg, beam)
    assert c.score_beams(first, sts, dirs, fld, cfg, beam).tobytes() == recs.tobytes() == R.score(first, sts, dirs, fld, cfg, beam, res).tobytes()
    for gate in (-7, cfg.max_dist + 1):
        odd = native.RRFieldConfig(cfg.width, cfg.height, cfg.cell, cfg.x0, cfg.y0, cfg.max_dist, gate, 0)
        assert np.array_equal(run_cast(c, sts, d_dirs, A, d_fld, odd, beam), ranges)
        assert c.score_beams(first, sts, dirs, fld, odd, beam).tobytes() == recs.tobytes()


def test_refusals_write_nothing():
    A = 16
    c = context(A, 0.1)
    L, h = c._L, c._h
    d = torch.full((8192,), GUARD, dtype=torch.uint8, device=DEV)
    p = d.data_ptr()
    q = p + 4096
    good = native.field_config(8, 8, 0.5, 0.0, 0.0, 4, 0)

    def grid(**kw):
        g = native.RRFieldConfig(good.width, good.height, good.cell, good.x0, good.y0, good.max_dist, good.gate, 0)
        for key, v in kw.items():
            setattr(g, key, v)
        return C.byref(g)

    def beam(**kw):
        b = native.RRBeamConfig(0, 64, 1, 2, 8, (C.c_int32 * 3)())
        for key, v in kw.items():
            if key.startswith("reserved"):
                b.reserved_[int(key[-1])] = v
            else:
                setattr(b, key, v)
        return C.byref(b)

    cast = lambda st=p, n=2, dr=p, fld=p, g=None, b=None, out=q: L.rr_cast_map_device(h, st, n, dr, fld, g or grid(), b or beam(), out, None)      # noqa: E731
    score = lambda fb=p, st=p, n=2, dr=p, fld=p, g=None, b=None, out=q: L.rr_score_beams_device(h, fb, st, n, dr, fld, g or grid(), b or beam(), out, None)   # noqa: E731
    prof = lambda pts=p, offs=p, n=2, mp=4, out=q: L.rr_scan_profile_device(h, pts, offs, n, mp, out, None)      # noqa: E731
    assert L.rr_cast_map_device(None, p, 2, p, p, grid(), beam(), q, None) == -1
    assert L.rr_score_beams_device(None, p, p, 2, p, p, grid(), beam(), q, None) == -1
    assert L.rr_scan_profile_device(None, p, p, 2, 4, q, None) == -1
    bare = native.Context(0)
    assert bare._L.rr_cast_map_device(bare._h, p, 2, p, p, grid(), beam(), q, None) == -2
    assert bare._L.rr_score_beams_device(bare._h, p, p, 2, p, p, grid(), beam(), q, None) == -2
    assert bare._L.rr_scan_profile_device(bare._h, p, p, 2, 4, q, None) == -2
    for kw in (dict(st=None), dict(dr=None), dict(fld=None), dict(out=None), dict(n=0), dict(n=65536), dict(st=p + 2), dict(dr=p + 2), dict(fld=p + 1),
               dict(out=q + 1)):
        assert cast(**kw) == -3 and b"rr_cast_map_device" in L.rr_last_error(h), kw
    for kw in (dict(fb=None), dict(st=None), dict(dr=None), dict(fld=None), dict(out=None), dict(n=0), dict(n=(1 << 22) + 1), dict(fb=p + 1),
               dict(out=q + 4)):
        assert score(**kw) == -3 and b"rr_score_beams_device" in L.rr_last_error(h), kw
    for kw in (dict(pts=None), dict(offs=None), dict(out=None), dict(n=0), dict(n=65536), dict(mp=-1), dict(mp=65537), dict(out=q + 1)):
        assert prof(**kw) == -3 and b"rr_scan_profile_device" in L.rr_last_error(h), kw
    for kw in (dict(bin_begin=-1), dict(bin_begin=65), dict(bin_end=R.N_CELLS + 1), dict(bin_step=0), dict(bin_step=65), dict(tol_bins=-1),
               dict(tol_bins=R.N_CELLS + 1), dict(clip_bins=-1), dict(clip_bins=R.N_CELLS + 1), dict(reserved0=1), dict(reserved1=1), dict(reserved2=-1)):
        assert cast(b=beam(**kw)) == -3 and score(b=beam(**kw)) == -3, kw
    for kw in (dict(width=0), dict(width=4097), dict(height=0), dict(height=4097), dict(cell=0.0), dict(cell=-0.5), dict(cell=float("nan")),
               dict(cell=float("inf")), dict(x0=float("inf")), dict(x0=float("nan")), dict(y0=float("-inf")), dict(y0=float("nan")), dict(max_dist=0),
               dict(max_dist=256)):
        assert cast(g=grid(**kw)) == -3 and score(g=grid(**kw)) == -3, kw
    assert L.rr_cast_map_device(h, p, 2, p, p, None, beam(), q, None) == -3 and L.rr_cast_map_device(h, p, 2, p, p, grid(), None, q, None) == -3
    assert L.rr_score_beams_device(h, p, p, 2, p, p, None, beam(), q, None) == -3 and L.rr_score_beams_device(h, p, p, 2, p, p, grid(), None, q, None) == -3
    torch.cuda.synchronize()
    assert bool((d == GUARD).all())
    # the host forms, on host buffers pre-filled with a pattern
    out = np.full(2 * A + 64, GUARD * 0x0101, np.uint16)
    st, dr, fld, fb = np.zeros((2, 4), np.float32), np.zeros((A, 2), np.float32), np.zeros((8, 8), np.uint16), np.zeros(A, np.uint16)
    pts, offs = np.zeros((2, 4), native.POINT_DTYPE), np.zeros((2, A + 1), np.uint32)
    for n, b in ((0, beam()), (65536, beam()), (2, beam(bin_step=0)), (2, beam(reserved1=7))):
        assert L.rr_cast_map(h, st.ctypes.data, n, dr.ctypes.data, fld.ctypes.data, grid(), b, out.ctypes.data) == -3
    for n, b in ((0, beam()), ((1 << 22) + 1, beam()), (2, beam(bin_end=R.N_CELLS + 1))):
        assert L.rr_score_beams(h, fb.ctypes.data, st.ctypes.data, n, dr.ctypes.data, fld.ctypes.data, grid(), b, out.ctypes.data) == -3
    for n, mp in ((0, 4), (65536, 4), (2, -1), (2, 65537)):
        assert L.rr_scan_profile(h, pts.ctypes.data, offs.ctypes.data, n, mp, out.ctypes.data) == -3
    assert L.rr_cast_map(bare._h, st.ctypes.data, 2, dr.ctypes.data, fld.ctypes.data, grid(), beam(), out.ctypes.data) == -2
    assert L.rr_score_beams(bare._h, fb.ctypes.data, st.ctypes.data, 2, dr.ctypes.data, fld.ctypes.data, grid(), beam(), out.ctypes.data) == -2
    assert L.rr_scan_profile(bare._h, pts.ctypes.data, offs.ctypes.data, 2, 4, out.ctypes.data) == -2
    for g in (grid(width=4097), grid(y0=float("nan")), grid(max_dist=0)):
        assert L.rr_cast_map(h, st.ctypes.data, 2, dr.ctypes.data, fld.ctypes.data, g, beam(), out.ctypes.data) == -3
        assert L.rr_score_beams(h, fb.ctypes.data, st.ctypes.data, 2, dr.ctypes.data, fld.ctypes.data, g, beam(), out.ctypes.data) == -3
    assert np.all(out == GUARD * 0x0101)


def loop_context():
    s, cfg = icp_ref.loop_scene(), icp_ref.loop_cfg()
    c = native.Context(0)
    c.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    c.set_materials(params.kaist_materials(), s["object_materials"], 0)
    c.set_config(cfg, icp_ref.LOOP_ANGLES)
    c.set_beam_samples(golden_beams(icp_ref.LOOP_SAMPLES))
    return c, cfg


def test_scoring_on_a_second_stream_beside_a_batch_in_flight():
    """cast_ref.stream_case"""
    c, rcfg = loop_context()
    A = icp_ref.LOOP_ANGLES
    case = R.stream_case()
    cfg, fld, dirs, states, first, beam = (case[k] for k in ("cfg", "field", "dirs", "states", "first", "beam"))
    assert np.array_equal(dirs, native.beam_directions(c._rrcfg)) and case["res"] == rcfg.resolution
    poses = np.stack([icp_ref.loop_pose((0.1 * j, 0.05 * j, 0.01 * j)) for j in range(8)])
    imgs = torch.zeros((8, rcfg.n_cells, A), dtype=torch.uint8, device=DEV)
    n = len(states)
    d_first, d_st, d_dirs, d_fld = dev(first), dev(states), dev(dirs), dev(fld)
    d_rec = torch.zeros(32 * n, dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()

    def enqueue(stream):
        c.score_beams_device(d_first.data_ptr(), d_st.data_ptr(), n, d_dirs.data_ptr(), d_fld.data_ptr(), cfg, beam, d_rec.data_ptr(), stream)

    c.simulate_batch_device(poses, imgs.data_ptr(), None)             # a batch in flight on the context's stream
    enqueue(side.cuda_stream)
    torch.cuda.synchronize()
    c.synchronize()
    beside = d_rec.cpu().numpy().tobytes()
    busy = imgs.cpu().numpy().copy()
    d_rec.zero_()
    torch.cuda.synchronize()
    enqueue(None)                                                    # alone, on the context's stream
    c.synchronize()
    alone = d_rec.cpu().numpy().tobytes()
    assert beside == alone == R.score(first, states, dirs, fld, cfg, beam, rcfg.resolution).tobytes()
    imgs.zero_()
    torch.cuda.synchronize()
    c.simulate_batch_device(poses, imgs.data_ptr(), None)
    c.synchronize()
    assert np.array_equal(imgs.cpu().numpy(), busy) and busy.any()   # ... and the batch beside it was not disturbed


# ---- 5. closed loop, 6. façade ------------------------------------------------------------------------------------------------------------------
def test_closed_loop_on_the_gpus_own_images():
    c, rcfg = loop_context()
    imgs = np.stack([c.simulate(icp_ref.loop_pose(p))[0] for p in O.LOOP_POSES + [icp_ref.LOOP_A, icp_ref.LOOP_B]])
    pts, offs = c.detect(imgs, icp_ref.LOOP_DET)
    cfg, st = F.loop_field_cfg(), O.loop_states()
    field_cfg = native.field_config(cfg.width, cfg.height, cfg.cell, cfg.x0, cfg.y0, R.LOOP_MAX_DIST, 0)
    ev = c.occupancy_update(pts[:8], offs[:8], cfg, O.LOOP_MODEL, st)
    fld = c.distance_field(c.occupancy_map(ev, cfg), field_cfg, R.LOOP_THRESHOLD)
    prof = c.scan_profile(pts[8:], offs[8:])
    assert np.array_equal(prof, R.profile(pts[8:], offs[8:], rcfg.n_cells, icp_ref.LOOP_ANGLES))
    dirs = native.beam_directions(c._rrcfg)
    beam = R.loop_beam(rcfg.resolution)
    states, xyz = F.loop_lattice()
    recs = c.score_beams(prof[1], states, dirs, fld, field_cfg, beam)
    assert recs.tobytes() == R.score(prof[1], states, dirs, fld, field_cfg, beam, rcfg.resolution).tobytes()
    wall = c.score_beams(prof[0], R.loop_behind_wall(), dirs, fld, field_cfg, beam)
    assert wall.tobytes() == R.score(prof[0], R.loop_behind_wall(), dirs, fld, field_cfg, beam, rcfg.resolution).tobytes()
    ranges = c.cast_map(states[:64], dirs, fld, field_cfg, beam)
    assert np.array_equal(ranges, R.brute(states[:64], dirs, fld, field_cfg, beam, rcfg.resolution))
    best = R.loop_check(recs, xyz, wall)
    print("closed loop on the GPU: argmax node (%.2f m, %.2f m, %.1f deg) %s; n_through at A %d, behind the wall %d"
          % (xyz[best][0], xyz[best][1], math.degrees(xyz[best][2]), recs[best], wall[0]["n_through"], wall[1]["n_through"]))


def test_radar_facade_casts_and_scores():
    s = icp_ref.loop_scene()
    r = radar.RadarHIP(s["verts"], s["faces"], s["face_object_id"])
    r.loadParams(params.kaist_materials(), s["object_materials"], 0)
    r.updateDynCfg(icp_ref.loop_cfg())
    r.setBeamSamples(golden_beams(icp_ref.LOOP_SAMPLES))
    poses = native.object_poses_array(np.stack([icp_ref.loop_pose(icp_ref.LOOP_A), icp_ref.loop_pose((-1.0, 0.5, math.radians(30.0)))]))
    base = F.loop_field_cfg()
    cfg = native.field_config(base.width, base.height, base.cell, base.x0, base.y0, R.LOOP_MAX_DIST, 0)
    fld = r.buildLikelihoodField(poses, cfg, icp_ref.LOOP_DET)
    clouds = r.simulatePointClouds(poses, **icp_ref.LOOP_DET)
    n_cells = icp_ref.loop_cfg().n_cells
    beam = native.beam_config(0, 280, n_cells, 1, 6, 24)
    states, _ = F.loop_lattice()
    states = states[:70]
    dirs = r.beamDirections()
    assert dirs.shape == (radar.N_ANGLES, 2) and dirs.dtype == np.float32
    prof = r.scanProfile(clouds[0])
    ranges = r.castMap(states, fld, cfg, beam)
    assert tuple(ranges.shape) == (70, radar.N_ANGLES) and ranges.is_cuda
    assert np.array_equal(ranges.cpu().numpy().view(np.uint16), r._ctx.cast_map(states, dirs, fld, cfg, beam))
    recs = r.scoreBeams(clouds[0], states, fld, cfg, beam)
    assert recs.tobytes() == r._ctx.score_beams(prof, states, dirs, fld, cfg, beam).tobytes()
    assert recs.tobytes() == R.score(prof, states, dirs, fld, cfg, beam, icp_ref.loop_cfg().resolution).tobytes()
    assert recs["n_cast"].max() > 0 and recs["n_agree"].max() > 0
