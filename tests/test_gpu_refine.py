"""Map refinement on the GPU (rr_refine.hip) against the numpy restatement of its definition (tests/refine_ref.py), byte for byte and with no
tolerance: the nearest-cell transform as u32 on degenerate and tile-edge grids, with empty, full, corner, lattice and random maps at four
saturations, and its invariant against the GPU's own distance field; the refinement's 48-byte records at the edges of its blocking, at every
iteration count, with both gates, with NaN, degenerate, off-grid and unnormalised states; the host forms; every refusal, with the output
buffers untouched; a call on a second stream beside a batch in flight; and a closed loop through the simulator."""
import math

import numpy as np
import pytest

import field_ref as F
import icp_ref
import refine_ref as R
from radarays_ros_amd import native, params, radar

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
N_ANGLES = 16
GUARD = 0xA5
REC = native.ICP_DTYPE.itemsize


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    c.set_config(params.kaist_preset(n_cells=64), N_ANGLES)
    return c


@pytest.fixture(scope="module")
def tiles():
    return native.refine_tile_sizes()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)


def guarded(n_bytes, fill=GUARD):
    return torch.full((n_bytes + 64,), fill, dtype=torch.uint8, device=DEV)


def payload(t, n_bytes):
    raw = t.cpu().numpy()
    assert np.all(raw[n_bytes:] == GUARD)                             # nothing behind the buffer
    return raw[:n_bytes].copy()


# ---- 1. the transform -----------------------------------------------------------------------------------------------------------------
def run_nearest(ctx, occ, cfg, threshold=1, stream=None, with_field=False):
    cells = cfg.width * cfg.height
    d_occ = dev(occ)
    d_out = guarded(4 * cells)
    d_fld = guarded(2 * cells)
    torch.cuda.synchronize()
    ctx.nearest_field_device(d_occ.data_ptr(), cfg, d_out.data_ptr(), threshold, stream)
    if with_field:
        ctx.distance_field_device(d_occ.data_ptr(), cfg, d_fld.data_ptr(), threshold, stream)
    torch.cuda.synchronize()
    near = payload(d_out, 4 * cells).view(np.uint32).reshape(cfg.height, cfg.width)
    if with_field:
        return near, payload(d_fld, 2 * cells).view(np.uint16).reshape(cfg.height, cfg.width)
    return near


@pytest.mark.parametrize("case", range(12))
def test_nearest_field_matches_the_restatement_and_the_gpus_distance_field(ctx, tiles, case):
    W, H = R.grid_list(tiles[2])[case]
    for name, occ in R.map_list(W, H).items():
        for md in R.MAX_DISTS:
            cfg = R.grid_cfg(W, H, md)
            got, fld = run_nearest(ctx, occ, cfg, with_field=True)
            assert got.tobytes() == R.nearest_field(occ, cfg).tobytes(), (W, H, name, md)
            some, d2 = R.nearest_d2(got, cfg)                         # the invariant: NONE iff the field is at cap2, else the field's value
            fld = fld.astype(np.int64)
            assert np.array_equal(some, fld < md * md) and np.array_equal(d2[some], fld[some]), (W, H, name, md)


def test_threshold_decides_what_is_occupied(ctx):
    rs = np.random.RandomState(5)
    occ = rs.choice(np.array([0, 1, 127, 128, 254, 255], np.uint8), (40, 70), p=[0.9, 0.02, 0.02, 0.02, 0.02, 0.02])
    cfg = R.grid_cfg(70, 40, 7)
    seen = []
    for th in (1, 128, 255):
        got = run_nearest(ctx, occ, cfg, th)
        assert got.tobytes() == R.nearest_field(occ, cfg, th).tobytes(), th
        seen.append(int((got.reshape(-1) == np.arange(got.size)).sum()))      # the cells that name themselves: the occupied ones
    assert seen[0] > seen[1] > seen[2] > 0


def test_the_host_form_of_the_transform_equals_the_device_form(ctx):
    occ = R.map_list(33, 65)["random1"]
    cfg = R.grid_cfg(33, 65, 255)
    assert ctx.nearest_field(occ, cfg).tobytes() == run_nearest(ctx, occ, cfg).tobytes()


# ---- 2. the refinement ------------------------------------------------------------------------------------------------------------------
GRID = dict(width=64, height=48, cell=0.3, x0=-9.6, y0=-7.2)       # negative x0 / y0, a cell that is not a power of two
MAX_DIST = 12
_INPUTS = {}


def inputs(gate):
    """a table and a scan, made once: walls and clutter on the grid, and a scan of 2 * points_tile + 40 points that samples the walls from
    a pose a little off, with points outside the grid and one that is not a point"""
    if gate not in _INPUTS:
        cfg = native.field_config(max_dist=MAX_DIST, gate=MAX_DIST if gate == "max" else 0, **GRID)
        rs = np.random.RandomState(40)
        occ = (rs.random_sample((cfg.height, cfg.width)) < 0.004).astype(np.uint8)
        occ[6, 5:58] = occ[41, 5:58] = 1
        occ[6:42, 5] = occ[6:42, 57] = 1
        occ[20:30, 30] = 1
        near = R.nearest_field(occ, cfg)
        m = 2 * native.refine_tile_sizes()[0] + 40
        on = R.cell_centres(rs.choice(np.nonzero(occ.reshape(-1))[0], m), cfg) + rs.uniform(-0.12, 0.12, (m, 2)).astype(np.float32)
        yaw, t = math.radians(-3.0), np.float32([-0.35, 0.25])       # the scan's own frame: the map seen from a pose a little off
        c, s = np.float32(math.cos(yaw)), np.float32(math.sin(yaw))
        scan = np.stack([c * on[:, 0] - s * on[:, 1], s * on[:, 0] + c * on[:, 1]], -1).astype(np.float32) + t
        scan[7] = (np.nan, 1.0)
        scan[11] = (40.0, 0.0)
        scan[12] = (0.0, -1e30)
        _INPUTS[gate] = (cfg, near, scan.astype(np.float32))
    return _INPUTS[gate]


def some_states(rs, n):
    """the identity, seeded small rotations and shifts around it, and -- from index 1 on -- one that throws every point off the grid, one with no
    direction, one with a NaN in its translation, one that is not normalised, one with a NaN direction, a half turn"""
    yaw = rs.uniform(-0.12, 0.12, n)
    st = native.se2_states(yaw, rs.uniform(-0.8, 0.8, n), rs.uniform(-0.8, 0.8, n))
    special = [(1.0, 0.0, 0.0, 0.0), (1.0, 0.0, 1000.0, 0.0), (0.0, 0.0, 0.3, 0.3), (1.0, 0.0, np.nan, 0.0), (2.4, 0.7, 0.1, -0.2),
               (np.nan, 1.0, 0.0, 0.0), (-1.0, 0.0, 0.0, 0.0), (np.inf, 0.0, 0.0, 0.0), (1e-200, 1e-200, 0.0, 0.1)]
    for k, row in enumerate(special[:n]):
        st[k] = row
    return np.ascontiguousarray(st, np.float64)


def run_refine(ctx, scan, count, max_points, states, near, cfg, iterations, stream=None):
    """the device form on guarded buffers -> the records as raw bytes.  `count` is what the device reads; the buffer holds max_points points"""
    pts = np.zeros(max(max_points, 1), native.POINT_DTYPE)
    m = min(len(scan), max_points)
    pts[:m] = R.points_of(scan[:m])
    n = len(states)
    d_pts, d_cnt, d_st, d_near = dev(pts), dev(np.array([count], np.uint32)), dev(states), dev(near)
    d_rec = guarded(REC * n)
    torch.cuda.synchronize()
    ctx.refine_poses_device(d_pts.data_ptr(), d_cnt.data_ptr(), max_points, d_st.data_ptr(), n, d_near.data_ptr(), cfg, d_rec.data_ptr(), iterations,
                            stream)
    torch.cuda.synchronize()
    return payload(d_rec, REC * n)


def check_refine(ctx, scan, count, max_points, states, near, cfg, iterations):
    got = run_refine(ctx, scan, count, max_points, states, near, cfg, iterations)
    want = R.refine(scan[:min(count, len(scan))], states, near, cfg, iterations, max_points)
    rec = got.view(native.ICP_DTYPE)
    assert got.tobytes() == want.tobytes(), (count, max_points, len(states), iterations, rec[:4], want[:4])
    return rec


def hyp_counts(tiles):
    return [1, tiles[1] - 1, tiles[1], tiles[1] + 1, 257]


def scan_counts(tiles):
    return [0, 1, tiles[0] - 1, tiles[0], tiles[0] + 1, 2 * tiles[0] + 1]


@pytest.mark.parametrize("gate", [0, "max"])
@pytest.mark.parametrize("k", range(5))
def test_refinement_at_every_hypothesis_count(ctx, tiles, k, gate):
    cfg, near, scan = inputs(gate)
    n = hyp_counts(tiles)[k]
    states = some_states(np.random.RandomState(50 + k), n)
    count = 2 * tiles[0] + 1
    rec = check_refine(ctx, scan, count, count, states, near, cfg, 10)
    assert rec["flags"][0] == 0 and rec["n_matched"][0] > (count // 2 if gate == "max" else 0)      # the comparison is not of empty sums
    if n > 8:
        init = states
        # thrown off the grid: DEGENERATE, nothing matched, the state unchanged
        assert rec["flags"][1] == R.DEGENERATE and rec["n_matched"][1] == 0 and (rec["tx"][1], rec["ty"][1], rec["c"][1]) == (1000.0, 0.0, 1.0)
        for h in (2, 5, 7, 8):                                       # no direction: the identity, flagged
            assert rec["flags"][h] & R.DEGENERATE, h
        assert rec["flags"][3] == R.DEGENERATE and np.isnan(rec["tx"][3]) and rec["n_matched"][3] == 0
        assert rec["flags"][4] == 0 and abs(math.hypot(rec["c"][4], rec["s"][4]) - 1.0) < 1e-15 and init[4][0] == 2.4
    if gate == "max" and n > 9:
        moved = np.abs(rec["tx"][9:] - states[9:, 2]) + np.abs(rec["ty"][9:] - states[9:, 3])
        assert np.all(moved > 0)                                      # ten iterations did move the ordinary states


@pytest.mark.parametrize("k", range(6))
def test_refinement_at_every_scan_count(ctx, tiles, k):
    cfg, near, scan = inputs("max")
    count = scan_counts(tiles)[k]
    states = some_states(np.random.RandomState(60 + k), tiles[1] + 1)
    rec = check_refine(ctx, scan, count, max(count, 1), states, near, cfg, 3)
    assert not np.any(rec["flags"] & R.TRUNCATED)
    if count == 0:
        assert np.all(rec["n_matched"] == 0) and np.all(rec["sse"] == 0) and np.all(rec["flags"] & R.DEGENERATE)
        assert np.all(check_refine(ctx, scan, 0, 1, states, near, cfg, 0)["flags"][[0, 1, 3, 4]] == 0)        # no solve ran
        cut = check_refine(ctx, scan, 5, 0, states, near, cfg, 1)    # max_points == 0: no point buffer at all, and a count above it
        assert np.all(cut["flags"] & R.TRUNCATED) and np.all(cut["n_matched"] == 0)
    if count > 1:                                                     # a count above max_points: the first max_points only, and flagged
        cut = check_refine(ctx, scan, count + 30, count - 1, states, near, cfg, 3)
        assert np.all(cut["flags"] & R.TRUNCATED) and cut.tobytes() != rec.tobytes()


@pytest.mark.parametrize("iterations", [0, 1, 10, 64])
def test_refinement_at_every_iteration_count(ctx, tiles, iterations):
    cfg, near, scan = inputs("max")
    states = some_states(np.random.RandomState(70), tiles[1] + 1)
    rec = check_refine(ctx, scan, len(scan), len(scan), states, near, cfg, iterations)
    if iterations == 0:                                               # the states as they stand, normalised; no solve, so no flag from one
        assert rec["flags"][1] == 0 and rec["flags"][3] == 0 and (rec["tx"][9], rec["ty"][9]) == (states[9][2], states[9][3])


def test_cell_centres_at_the_identity_cost_nothing(ctx):
    cfg, near, _ = inputs("max")
    index = np.unique(near[near != R.NONE])[:150]
    scan = R.cell_centres(index, cfg)
    rec = check_refine(ctx, scan, len(scan), len(scan), native.se2_states([0.0, 0.0], [0.0, 0.05], [0.0, -0.04]), near, cfg, 2)
    assert rec["sse"][0] == 0 and rec["n_matched"][0] == len(scan) and (rec["c"][0], rec["s"][0], rec["tx"][0], rec["ty"][0]) == (1.0, 0.0, 0.0, 0.0)
    assert rec["sse"][1] == 0 and rec["n_matched"][1] == len(scan)


def test_the_host_form_of_the_refinement_equals_the_device_form(ctx, tiles):
    cfg, near, scan = inputs("max")
    states = some_states(np.random.RandomState(80), tiles[1] + 3)
    got = ctx.refine_poses(R.points_of(scan), states, near, cfg, 5)
    assert got.tobytes() == run_refine(ctx, scan, len(scan), len(scan), states, near, cfg, 5).tobytes()
    none = ctx.refine_poses(R.points_of(scan[:0]), states, near, cfg, 0)
    assert np.all(none["n_matched"] == 0) and none.tobytes() == R.refine(scan[:0], states, near, cfg, 0).tobytes()


# ---- 3. refusals: one call per rule, nothing written ------------------------------------------------------------------------------------
def test_refusals_write_nothing(ctx):
    L, h = ctx._L, ctx._h
    import ctypes as C
    d = torch.full((4096,), GUARD, dtype=torch.uint8, device=DEV)
    p = d.data_ptr()
    q = p + 2048
    good = native.field_config(8, 8, 0.5, 0.0, 0.0, 4, 2)

    def cfg(**kw):
        g = native.RRFieldConfig(good.width, good.height, good.cell, good.x0, good.y0, good.max_dist, good.gate, 0)
        for k, v in kw.items():
            setattr(g, k, v)
        return C.byref(g)

    bad_cfgs = [dict(width=0), dict(width=4097), dict(height=0), dict(height=4097), dict(cell=0.0), dict(cell=-0.5), dict(cell=float("nan")),
                dict(cell=float("inf")), dict(x0=float("nan")), dict(y0=float("-inf")), dict(max_dist=0), dict(max_dist=256), dict(gate=-1), dict(gate=5)]
    far_cfgs = [dict(x0=8192.0), dict(y0=-8192.0), dict(x0=8188.0), dict(y0=8188.0), dict(x0=-1e6), dict(width=4096, cell=4.0, x0=-8191.0)]
    near = lambda occ=p, th=1, g=None, out=q: L.rr_nearest_field_device(h, occ, th, g or cfg(), out, None)                                            # noqa: E731
    ref = lambda pts=p, cnt=p, mp=4, st=p, n=2, tab=p, g=None, it=3, rec=q: L.rr_refine_poses_device(h, pts, cnt, mp, st, n, tab, g or cfg(), it, rec, None)  # noqa: E731
    assert L.rr_nearest_field_device(None, p, 1, cfg(), q, None) == -1
    assert L.rr_refine_poses_device(None, p, p, 4, p, 2, p, cfg(), 3, q, None) == -1
    for kw in (dict(occ=None), dict(out=None), dict(th=0), dict(th=256), dict(out=p), dict(out=q + 2)):
        assert near(**kw) == -3 and b"rr_nearest_field_device" in L.rr_last_error(h), kw
    for kw in (dict(pts=None), dict(cnt=None), dict(st=None), dict(tab=None), dict(rec=None), dict(mp=-1), dict(mp=65537), dict(n=0), dict(n=(1 << 22) + 1),
               dict(it=-1), dict(it=65), dict(st=p + 4), dict(rec=q + 4), dict(tab=p + 2)):
        assert ref(**kw) == -3 and b"rr_refine_poses_device" in L.rr_last_error(h), kw
    for kw in bad_cfgs:
        assert near(g=cfg(**kw)) == -3 and ref(g=cfg(**kw)) == -3, kw
    for kw in far_cfgs:
        assert ref(g=cfg(**kw)) == -3 and b"8192" in L.rr_last_error(h), kw
    assert L.rr_nearest_field_device(h, p, 1, None, q, None) == -3 and L.rr_refine_poses_device(h, p, p, 4, p, 2, p, None, 3, q, None) == -3
    torch.cuda.synchronize()
    assert bool((d == GUARD).all())
    # the host forms, on host buffers pre-filled with a pattern
    occ = np.zeros((8, 8), np.uint8)
    tab = np.full((8, 8), GUARD * 0x01010101, np.uint32)
    rec = np.full(2 * REC, GUARD, np.uint8)
    pts = np.zeros(4, native.POINT_DTYPE)
    st = np.zeros((2, 4), np.float64)
    for th, g in ((0, cfg()), (256, cfg()), (1, cfg(max_dist=256))):
        assert L.rr_nearest_field(h, occ.ctypes.data, th, g, tab.ctypes.data) == -3
    for n, it, g in ((0, 3, cfg()), ((1 << 22) + 1, 3, cfg()), (2, 65, cfg()), (2, 3, cfg(gate=5)), (2, 3, cfg(x0=8190.0))):
        assert L.rr_refine_poses(h, pts.ctypes.data, 4, 4, st.ctypes.data, n, tab.ctypes.data, g, it, rec.ctypes.data) == -3
    assert np.all(tab == GUARD * 0x01010101) and np.all(rec == GUARD)
    bare = native.Context(0)                                          # no radar config is needed: the shape comes with the call
    assert bare.nearest_field(occ, good).tobytes() == np.full((8, 8), R.NONE, np.uint32).tobytes()


# ---- 4. two streams ---------------------------------------------------------------------------------------------------------------------
def loop_context():
    from common import golden_beams
    s, cfg = icp_ref.loop_scene(), icp_ref.loop_cfg()
    c = native.Context(0)
    c.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    c.set_materials(params.kaist_materials(), s["object_materials"], 0)
    c.set_config(cfg, icp_ref.LOOP_ANGLES)
    c.set_beam_samples(golden_beams(icp_ref.LOOP_SAMPLES))
    return c, cfg


def test_refinement_on_a_second_stream_beside_a_batch_in_flight(tiles):
    c, rcfg = loop_context()
    A = icp_ref.LOOP_ANGLES
    cfg, near, scan = inputs("max")
    states = some_states(np.random.RandomState(90), 4 * tiles[1] + 5)
    poses = np.stack([icp_ref.loop_pose((0.1 * k, 0.05 * k, 0.01 * k)) for k in range(8)])
    imgs = torch.zeros((8, rcfg.n_cells, A), dtype=torch.uint8, device=DEV)
    n = len(states)
    d_pts, d_cnt, d_st, d_near = dev(R.points_of(scan)), dev(np.array([len(scan)], np.uint32)), dev(states), dev(near)
    d_rec = torch.zeros(REC * n, dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()

    def enqueue(stream):
        c.refine_poses_device(d_pts.data_ptr(), d_cnt.data_ptr(), len(scan), d_st.data_ptr(), n, d_near.data_ptr(), cfg, d_rec.data_ptr(), 10, stream)

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
    assert beside == alone == R.refine(scan, states, near, cfg, 10).tobytes()
    imgs.zero_()
    torch.cuda.synchronize()
    c.simulate_batch_device(poses, imgs.data_ptr(), None)
    c.synchronize()
    assert np.array_equal(imgs.cpu().numpy(), busy) and busy.any()   # ... and the batch beside it was not disturbed


# ---- 5. closed loop ---------------------------------------------------------------------------------------------------------------------
def test_closed_loop_a_scan_is_refined_against_the_map_from_the_keyframes_own_state():
    c, _ = loop_context()
    imgs = np.stack([c.simulate(icp_ref.loop_pose(p))[0] for p in (icp_ref.LOOP_A, icp_ref.LOOP_B)])
    pts, offs = c.detect(imgs, icp_ref.LOOP_DET)
    assert len(pts[0]) >= 100 and len(pts[1]) >= 100
    cfg = R.loop_field_cfg()
    occ = c.rasterize_points([pts[0]], offs[:1], cfg, F.loop_map_state())
    near = c.nearest_field(occ, cfg)
    assert near.tobytes() == R.nearest_field(occ, cfg).tobytes()
    rec = c.refine_poses(pts[1], R.loop_guess(), near, cfg, R.LOOP_ITERATIONS)
    assert rec.tobytes() == R.refine(pts[1], R.loop_guess(), near, cfg, R.LOOP_ITERATIONS).tobytes()       # the restatement on the GPU's own images
    eyaw, et = R.loop_errors(rec[0])
    print("closed loop on the GPU: from A's own state (%.3f deg, %.4f m off) %d iterations at gate %d end %.4f deg and %.4f m off the truth, sse %d "
          "over %d pairs" % (math.degrees(R.LOOP_GUESS_YAW), R.LOOP_GUESS_T, R.LOOP_ITERATIONS, R.LOOP_GATE, math.degrees(eyaw), et, rec[0]["sse"],
                             rec[0]["n_matched"]))
    assert rec[0]["flags"] == 0
    assert eyaw < R.LOOP_GUESS_YAW and et < R.LOOP_GUESS_T            # the result beats the guess in both
    assert eyaw <= R.LOOP_YAW_BOUND and et <= R.LOOP_T_BOUND          # twice the host figure in each


def test_radar_facade_builds_a_table_and_refines_poses():
    from common import golden_beams
    s = icp_ref.loop_scene()
    r = radar.RadarHIP(s["verts"], s["faces"], s["face_object_id"])
    r.loadParams(params.kaist_materials(), s["object_materials"], 0)
    r.updateDynCfg(icp_ref.loop_cfg())
    r.setBeamSamples(golden_beams(icp_ref.LOOP_SAMPLES))
    poses = native.object_poses_array(np.stack([icp_ref.loop_pose(icp_ref.LOOP_A), icp_ref.loop_pose(icp_ref.LOOP_B)]))
    clouds = r.simulatePointClouds(poses, **icp_ref.LOOP_DET)
    cfg = R.loop_field_cfg()
    occ = F.rasterize([clouds[0]], cfg, F.loop_map_state())
    table = r.buildNearestField(occ, cfg)
    assert table.is_cuda and table.dtype == torch.int32 and tuple(table.shape) == (cfg.height, cfg.width)
    near = table.cpu().numpy().view(np.uint32)
    assert near.tobytes() == R.nearest_field(occ, cfg).tobytes()
    states32, _ = F.loop_lattice()                                    # float32 states of the lattice: widened to f64 on the device
    states32 = states32[::37]
    out = r.refinePoses(clouds[1], torch.from_numpy(states32).to(DEV), table, cfg, 4)
    assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (len(states32), 6)
    rec = radar.RadarHIP.refineRecords(out)
    assert rec.tobytes() == R.refine(clouds[1], states32.astype(np.float64), near, cfg, 4).tobytes()
    assert np.array_equal(out[:, :4].cpu().numpy(), np.stack([rec["c"], rec["s"], rec["tx"], rec["ty"]], -1))
    again = radar.RadarHIP.refineRecords(r.refinePoses(clouds[1], states32.astype(np.float64), near, cfg, 4))     # host arrays pass too
    assert again.tobytes() == rec.tobytes()
