"""The likelihood field on the GPU (rr_field.hip) against the numpy restatement of its definition (tests/field_ref.py), bit for bit: the
distance transform on degenerate, odd and tile-edge grids, with empty, full, single-cell, equidistant and random maps at four saturations
and three thresholds; the rasteriser on cell edges, outside every side, with NaN and infinite coordinates, truncated and empty frames,
accumulating calls and states; the scorer at the edges of its blocking, with records compared as raw bytes; every refusal, with the output
buffers untouched; a scoring call on a second stream beside a batch in flight; and a closed loop through the simulator in which a lattice
search finds the pose of a scan in a map within the figure test_field_host.py measured plus one lattice step."""
import math

import numpy as np
import pytest

import field_ref as F
import icp_ref
from common import golden_beams
from radarays_ros_amd import native, params, radar

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
N_ANGLES = 16
GUARD = 0xA5


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    c.set_config(params.kaist_preset(n_cells=64), N_ANGLES)
    return c


@pytest.fixture(scope="module")
def tiles():
    return native.field_tile_sizes()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)


def guarded(n_bytes, fill=GUARD):
    return torch.full((n_bytes + 64,), fill, dtype=torch.uint8, device=DEV)


def payload(t, n_bytes):
    raw = t.cpu().numpy()
    assert np.all(raw[n_bytes:] == GUARD)                             # nothing behind the buffer
    return raw[:n_bytes].copy()


# ---- 1. the distance transform ------------------------------------------------------------------------------------------------
def run_field(ctx, occ, cfg, threshold=1, stream=None):
    d_occ = dev(occ)
    d_out = guarded(2 * cfg.width * cfg.height)
    torch.cuda.synchronize()
    ctx.distance_field_device(d_occ.data_ptr(), cfg, d_out.data_ptr(), threshold, stream)
    torch.cuda.synchronize()
    return payload(d_out, 2 * cfg.width * cfg.height).view(np.uint16).reshape(cfg.height, cfg.width)


@pytest.mark.parametrize("case", range(8))
def test_distance_field_matches_the_restatement(ctx, tiles, case):
    W, H = F.grid_list(tiles[2])[case]
    for name, occ in F.map_list(W, H).items():
        for md in F.MAX_DISTS:
            cfg = F.grid_cfg(W, H, md)
            got = run_field(ctx, occ, cfg)
            assert np.array_equal(got, F.distance_field(occ, cfg)), (W, H, name, md)


def test_the_saturation_ring_of_a_lone_cell(ctx):
    occ = np.zeros((65, 33), np.uint8)
    occ[30, 16] = 1
    got = run_field(ctx, occ, F.grid_cfg(33, 65, 3)).astype(np.int64)
    iy, ix = np.mgrid[0:65, 0:33]
    assert np.array_equal(got, np.minimum(9, (iy - 30) ** 2 + (ix - 16) ** 2))


def test_threshold_decides_what_is_occupied(ctx):
    rs = np.random.RandomState(5)
    occ = rs.choice(np.array([0, 1, 127, 128, 254, 255], np.uint8), (40, 70), p=[0.9, 0.02, 0.02, 0.02, 0.02, 0.02])
    cfg = F.grid_cfg(70, 40, 7)
    seen = []
    for th in (1, 128, 255):
        got = run_field(ctx, occ, cfg, th)
        assert np.array_equal(got, F.distance_field(occ, cfg, th)), th
        seen.append(int((got == 0).sum()))
    assert seen[0] > seen[1] > seen[2] > 0


def test_the_host_form_of_the_transform_equals_the_device_form(ctx):
    occ = F.map_list(33, 65)["random1"]
    cfg = F.grid_cfg(33, 65, 255)
    assert np.array_equal(ctx.distance_field(occ, cfg), run_field(ctx, occ, cfg))


# ---- 2. the rasteriser --------------------------------------------------------------------------------------------------------------
def run_raster(ctx, clouds, cfg, states=None, max_points=None, occ=None, stream=None):
    """the device form on guarded buffers -> uint8 [height][width].  A cloud longer than max_points keeps its true total in the offsets"""
    n = len(clouds)
    mp = max(1, max(len(c) for c in clouds)) if max_points is None else max_points
    pts = np.zeros((n, max(mp, 1)), native.POINT_DTYPE)
    offs = np.zeros((n, N_ANGLES + 1), np.uint32)
    for f, c in enumerate(clouds):
        pts[f, :min(len(c), mp)] = F.points_of(c[:mp])
        offs[f, 1:] = len(c)
    cells = cfg.width * cfg.height
    d_occ = guarded(cells)
    d_occ[:cells] = 0 if occ is None else dev(occ)
    d_pts, d_offs = dev(pts), dev(offs)
    d_st = None if states is None else dev(np.ascontiguousarray(states, np.float64))
    torch.cuda.synchronize()
    ctx.rasterize_points_device(d_pts.data_ptr(), d_offs.data_ptr(), n, mp, cfg, d_occ.data_ptr(), None if d_st is None else d_st.data_ptr(), stream)
    torch.cuda.synchronize()
    return payload(d_occ, cells).reshape(cfg.height, cfg.width)


def edge_cloud(cfg):
    """points exactly on cell edges (x = x0 + k * cell in f32, cell not a power of two), just outside each of the four sides, and points that
    are not points"""
    cell, x0, y0 = np.float32(cfg.cell), np.float32(cfg.x0), np.float32(cfg.y0)
    k = np.arange(-1, cfg.width + 2, dtype=np.float32)
    on_x = np.stack([x0 + k * cell, np.full(len(k), y0 + np.float32(1.5) * cell, np.float32)], -1)
    j = np.arange(-1, cfg.height + 2, dtype=np.float32)
    on_y = np.stack([np.full(len(j), x0 + np.float32(2.5) * cell, np.float32), y0 + j * cell], -1)
    hi_x, hi_y = x0 + np.float32(cfg.width) * cell, y0 + np.float32(cfg.height) * cell
    up, down = (lambda v: np.nextafter(np.float32(v), np.float32(np.inf))), (lambda v: np.nextafter(np.float32(v), np.float32(-np.inf)))
    mid_x, mid_y = x0 + np.float32(3.25) * cell, y0 + np.float32(3.25) * cell
    sides = np.float32([[down(x0), mid_y], [x0, mid_y], [hi_x, mid_y], [down(hi_x), mid_y], [up(hi_x), mid_y],
                        [mid_x, down(y0)], [mid_x, y0], [mid_x, hi_y], [mid_x, down(hi_y)], [mid_x, up(hi_y)]])
    odd = np.float32([[np.nan, mid_y], [mid_x, np.nan], [np.inf, mid_y], [mid_x, -np.inf], [-np.inf, np.inf], [1e30, mid_y], [mid_x, -1e30]])
    return np.concatenate([on_x, on_y, sides, odd]).astype(np.float32)


RASTER_CFG = dict(width=21, height=13, cell=0.3, x0=-2.1, y0=-1.7)      # negative x0 / y0, a cell that is not a power of two


def test_rasteriser_on_cell_edges_outside_and_on_points_that_are_not_points(ctx):
    cfg = native.field_config(max_dist=5, **RASTER_CFG)
    cloud = edge_cloud(cfg)
    got = run_raster(ctx, [cloud], cfg)
    want = F.rasterize([cloud], cfg)
    assert np.array_equal(got, want)
    assert want.sum() > (cfg.width + cfg.height) // 2 and set(np.unique(got)) == {0, 1}
    inside, _ = F.cells(cloud[:, 0], cloud[:, 1], cfg)
    assert 0 < inside.sum() < len(cloud)                              # both kinds are there


def test_rasteriser_truncated_empty_and_accumulating_frames(ctx):
    cfg = native.field_config(max_dist=5, **RASTER_CFG)
    rs = np.random.RandomState(21)
    a, b, none = (rs.uniform(-3, 5, (m, 2)).astype(np.float32) for m in (300, 77, 0))
    got = run_raster(ctx, [a, none, b], cfg, max_points=256)          # a's true count exceeds max_points: its first 256 only
    assert np.array_equal(got, F.rasterize([a, none, b], cfg, max_points=256))
    assert not np.array_equal(got, F.rasterize([a, none, b], cfg)) and got.sum() > 50
    assert run_raster(ctx, [none], cfg).sum() == 0                    # a frame with count 0 writes nothing
    both = run_raster(ctx, [a, b], cfg)
    twice = run_raster(ctx, [b], cfg, occ=run_raster(ctx, [a], cfg))
    assert np.array_equal(both, twice) and np.array_equal(both, F.rasterize([a, b], cfg))
    assert np.array_equal(run_raster(ctx, [b, a], cfg), both)         # whatever the order


def test_rasteriser_states(ctx):
    cfg = native.field_config(max_dist=5, **RASTER_CFG)
    rs = np.random.RandomState(22)
    a, b = (rs.uniform(-3, 5, (m, 2)).astype(np.float32) for m in (257, 64))
    a[5] = (np.inf, 0.0)                                              # 0 * inf under the identity: NaN either way
    ident = native.se2_states([0.0, 0.0])
    null = run_raster(ctx, [a, b], cfg)
    assert np.array_equal(run_raster(ctx, [a, b], cfg, ident), null) and np.array_equal(null, F.rasterize([a, b], cfg, ident))
    quarter = np.array([[0.0, 1.0, 0.25, -0.5], [0.0, 1.0, 0.0, 0.0]])          # c = 0, s = 1: (x, y) -> (-y, x)
    got = run_raster(ctx, [a, b], cfg, quarter)
    assert np.array_equal(got, F.rasterize([a, b], cfg, quarter)) and not np.array_equal(got, null)
    turned = np.stack([-b[:, 1], b[:, 0]], -1)
    assert np.array_equal(run_raster(ctx, [b], cfg, quarter[1:]), run_raster(ctx, [turned], cfg))
    mixed = native.se2_states([0.3, -2.0], [0.7, -0.2], [1e-3, 4.0]) * np.array([[1.0, 1.0, 1.0, 1.0], [1.3, 1.3, 1.0, 1.0]])    # not normalised: used as given
    assert np.array_equal(run_raster(ctx, [a, b], cfg, mixed), F.rasterize([a, b], cfg, mixed))
    assert np.array_equal(run_raster(ctx, [a], cfg, np.array([[np.nan, 0.0, 0.0, 0.0]])), np.zeros((cfg.height, cfg.width), np.uint8))


def test_the_host_form_of_the_rasteriser_equals_the_device_form(ctx):
    cfg = native.field_config(max_dist=5, **RASTER_CFG)
    rs = np.random.RandomState(23)
    a, b = (rs.uniform(-3, 5, (m, 2)).astype(np.float32) for m in (90, 31))
    st = native.se2_states([0.2, -0.1], [0.5, 0.0], [0.0, -0.5])
    offs = np.zeros((2, N_ANGLES + 1), np.uint32)
    offs[:, -1] = (90, 31)
    first = ctx.rasterize_points([F.points_of(a)], offs[:1], cfg, st[:1])
    kept = first.copy()
    both = ctx.rasterize_points([F.points_of(b)], offs[1:], cfg, st[1:], occ=first)
    assert np.array_equal(first, kept)
    assert np.array_equal(both, run_raster(ctx, [a, b], cfg, st)) and np.array_equal(both, ctx.rasterize_points([F.points_of(a), F.points_of(b)], offs, cfg, st))


# ---- 3. the scorer ------------------------------------------------------------------------------------------------------------------
SCORE_GRID = dict(width=64, height=48, cell=0.3, x0=-9.6, y0=-7.2)
_SCORE = {}


def score_inputs(gate):
    """a field and a scan, made once: the field of a 1 % map, a scan of 2 * points_tile + 40 points in and around the grid"""
    if gate not in _SCORE:
        md = 12
        cfg = native.field_config(max_dist=md, gate=md if gate == "max" else 0, **SCORE_GRID)
        rs = np.random.RandomState(40)
        occ = (rs.random_sample((cfg.height, cfg.width)) < 0.01).astype(np.uint8)
        fld = F.distance_field(occ, cfg)
        scan = rs.uniform(-8, 8, (2 * native.field_tile_sizes()[0] + 40, 2)).astype(np.float32)
        scan[7] = (np.nan, 1.0)
        _SCORE[gate] = (cfg, fld, scan)
    return _SCORE[gate]


def some_states(rs, n):
    """the identity, seeded random rotations and shifts, one that moves every point outside the grid, one that holds a NaN, and one that puts
    points on cell edges (a shift of a whole number of cells for a scan whose points sit on multiples of the cell)"""
    st = native.pose_lattice((0.0, 0.0, 0.0), 0.0, 1.0, 0.0, 1.0)[0].repeat(n, axis=0)
    yaw = rs.uniform(-math.pi, math.pi, n)
    st[:, 0], st[:, 1] = np.cos(yaw), np.sin(yaw)
    st[:, 2:] = rs.uniform(-3, 3, (n, 2))
    st[0] = (1.0, 0.0, 0.0, 0.0)
    if n > 1:
        st[1] = (1.0, 0.0, 1000.0, 0.0)
    if n > 2:
        st[2] = (np.nan, 0.0, 0.0, 0.0)
    if n > 3:
        st[3] = (1.0, 0.0, np.float32(0.3) * 3, np.float32(0.3) * -2)
    if n > 4:
        st[4] = (0.0, 1.0, 0.0, np.nan)
    return np.ascontiguousarray(st, np.float32)


def run_score(ctx, scan, count, max_points, states, fld, cfg, stream=None, offset_bytes=0):
    """the device form on guarded buffers -> the records as raw bytes.  `count` is what the device reads; the buffer holds max_points points"""
    pts = np.zeros(max(max_points, 1), native.POINT_DTYPE)
    m = min(len(scan), max_points)
    pts[:m] = F.points_of(scan[:m])
    n = len(states)
    d_pts, d_cnt, d_st, d_fld = dev(pts), dev(np.array([count], np.uint32)), dev(states), dev(fld)
    d_rec = guarded(16 * n)
    torch.cuda.synchronize()
    ctx.score_poses_device(d_pts.data_ptr(), d_cnt.data_ptr(), max_points, d_st.data_ptr(), n, d_fld.data_ptr(), cfg, d_rec.data_ptr(), stream)
    torch.cuda.synchronize()
    return payload(d_rec, 16 * n)


def check_score(ctx, scan, count, max_points, states, fld, cfg):
    got = run_score(ctx, scan, count, max_points, states, fld, cfg)
    want = F.score(scan[:min(count, len(scan))], states, fld, cfg, max_points)
    assert got.tobytes() == want.tobytes(), (count, max_points, len(states), got.view(native.FIELD_DTYPE)[:4], want[:4])
    return got.view(native.FIELD_DTYPE)


def hyp_counts(tiles):
    return [1, 63, 64, 65, tiles[1] - 1, tiles[1], tiles[1] + 1, 1000]


def scan_counts(tiles):
    return [0, 1, tiles[0] - 1, tiles[0], tiles[0] + 1, 2 * tiles[0] + 1]


@pytest.mark.parametrize("gate", [0, "max"])
@pytest.mark.parametrize("k", range(8))
def test_scorer_at_every_hypothesis_count(ctx, tiles, k, gate):
    cfg, fld, scan = score_inputs(gate)
    n = hyp_counts(tiles)[k]
    states = some_states(np.random.RandomState(50 + k), n)
    count = 2 * tiles[0] + 1
    rec = check_score(ctx, scan, count, count, states, fld, cfg)
    cap2 = cfg.max_dist ** 2
    assert rec["n_in"][0] > count // 2                                # the comparison is not of empty sums
    if n > 2:
        assert (rec["sum_d2"][1], rec["n_in"][1], rec["n_hit"][1]) == (count * cap2, 0, 0) == (rec["sum_d2"][2], rec["n_in"][2], rec["n_hit"][2])
    if gate == "max":
        assert np.array_equal(rec["n_hit"], rec["n_in"])              # every field value is <= cap2
    else:
        assert rec["n_hit"][0] < rec["n_in"][0]


@pytest.mark.parametrize("k", range(6))
def test_scorer_at_every_scan_count(ctx, tiles, k):
    cfg, fld, scan = score_inputs(0)
    count = scan_counts(tiles)[k]
    states = some_states(np.random.RandomState(60 + k), tiles[1] + 1)
    rec = check_score(ctx, scan, count, max(count, 1), states, fld, cfg)
    if count == 0:
        assert np.all(rec.view(np.uint8) == 0)
    # a count above max_points: the first max_points only
    if count > 1:
        cut = check_score(ctx, scan, count + 30, count - 1, states, fld, cfg)
        assert cut.tobytes() != rec.tobytes()
    # max_points == 0: no point buffer at all
    if count == 0:
        assert np.all(run_score(ctx, scan, 5, 0, states, fld, cfg) == 0)


def test_scorer_with_points_on_cell_edges(ctx):
    cfg, fld, _ = score_inputs(0)
    cell, x0, y0 = np.float32(cfg.cell), np.float32(cfg.x0), np.float32(cfg.y0)
    kx, ky = np.meshgrid(np.arange(-1, cfg.width + 2, 3, dtype=np.float32), np.arange(-1, cfg.height + 2, 3, dtype=np.float32))
    scan = np.stack([(x0 + kx * cell).ravel(), (y0 + ky * cell).ravel()], -1).astype(np.float32)
    shift = lambda i, j: (1.0, 0.0, np.float32(i) * cell, np.float32(j) * cell)   # noqa: E731
    states = np.float32([shift(0, 0), shift(1, 0), shift(0, -1), shift(-2, 5), (0.0, 1.0, 0.0, 0.0), (-1.0, 0.0, 0.0, 0.0)])
    rec = check_score(ctx, scan, len(scan), len(scan), states, fld, cfg)
    assert 0 < rec["n_in"][0] < len(scan)


def test_the_host_form_of_the_scorer_equals_the_device_form(ctx, tiles):
    cfg, fld, scan = score_inputs(0)
    states = some_states(np.random.RandomState(70), tiles[1] + 3)
    got = ctx.score_poses(F.points_of(scan), states, fld, cfg)
    assert got.tobytes() == run_score(ctx, scan, len(scan), len(scan), states, fld, cfg).tobytes()
    assert ctx.score_poses(F.points_of(scan[:0]), states, fld, cfg).tobytes() == bytes(16 * len(states))


# ---- 4. refusals: one call per rule, nothing written ------------------------------------------------------------------------------------
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
    ras = lambda pts=p, offs=p, n=2, mp=4, st=None, g=None, occ=q: L.rr_rasterize_points_device(h, pts, offs, n, mp, st, g or cfg(), occ, None)   # noqa: E731
    dist = lambda occ=p, th=1, g=None, fld=q: L.rr_distance_field_device(h, occ, th, g or cfg(), fld, None)                                       # noqa: E731
    sco = lambda pts=p, cnt=p, mp=4, st=p, n=2, fld=p, g=None, rec=q: L.rr_score_poses_device(h, pts, cnt, mp, st, n, fld, g or cfg(), rec, None)  # noqa: E731
    assert L.rr_rasterize_points_device(None, p, p, 2, 4, None, cfg(), q, None) == -1
    assert L.rr_distance_field_device(None, p, 1, cfg(), q, None) == -1
    assert L.rr_score_poses_device(None, p, p, 4, p, 2, p, cfg(), q, None) == -1
    bare = native.Context(0)
    assert bare._L.rr_rasterize_points_device(bare._h, p, p, 2, 4, None, cfg(), q, None) == -2
    for kw in (dict(pts=None), dict(offs=None), dict(occ=None), dict(n=0), dict(n=65536), dict(mp=-1), dict(mp=65537), dict(st=p + 4)):
        assert ras(**kw) == -3 and b"rr_rasterize_points_device" in L.rr_last_error(h), kw
    for kw in (dict(occ=None), dict(fld=None), dict(th=0), dict(th=256), dict(fld=p)):
        assert dist(**kw) == -3 and b"rr_distance_field_device" in L.rr_last_error(h), kw
    for kw in (dict(pts=None), dict(cnt=None), dict(st=None), dict(fld=None), dict(rec=None), dict(mp=-1), dict(mp=65537), dict(n=0), dict(n=(1 << 22) + 1),
               dict(st=p + 2), dict(rec=q + 4)):
        assert sco(**kw) == -3 and b"rr_score_poses_device" in L.rr_last_error(h), kw
    for kw in bad_cfgs:
        assert ras(g=cfg(**kw)) == -3 and dist(g=cfg(**kw)) == -3 and sco(g=cfg(**kw)) == -3, kw
    assert L.rr_rasterize_points_device(h, p, p, 2, 4, None, None, q, None) == -3 and L.rr_distance_field_device(h, p, 1, None, q, None) == -3
    assert L.rr_score_poses_device(h, p, p, 4, p, 2, p, None, q, None) == -3
    torch.cuda.synchronize()
    assert bool((d == GUARD).all())
    # the host forms, on host buffers pre-filled with a pattern
    occ = np.full((8, 8), GUARD, np.uint8)
    fld = np.full((8, 8), GUARD * 0x0101, np.uint16)
    rec = np.full(2 * 16, GUARD, np.uint8)
    pts = np.zeros((2, 4), native.POINT_DTYPE)
    offs = np.zeros((2, N_ANGLES + 1), np.uint32)
    st = np.zeros((2, 4), np.float32)
    for kw in (dict(n=0), dict(n=65536), dict(mp=65537), dict(mp=-1), dict(g=cfg(cell=0.0))):
        a = dict(n=2, mp=4, g=cfg())
        a.update(kw)
        assert L.rr_rasterize_points(h, pts.ctypes.data, offs.ctypes.data, a["n"], a["mp"], None, a["g"], occ.ctypes.data) == -3, kw
    assert L.rr_rasterize_points(bare._h, pts.ctypes.data, offs.ctypes.data, 2, 4, None, cfg(), occ.ctypes.data) == -2
    for th, g in ((0, cfg()), (256, cfg()), (1, cfg(max_dist=256))):
        assert L.rr_distance_field(h, occ.ctypes.data, th, g, fld.ctypes.data) == -3
    for n, g in ((0, cfg()), ((1 << 22) + 1, cfg()), (2, cfg(gate=5))):
        assert L.rr_score_poses(h, pts.ctypes.data, 4, 4, st.ctypes.data, n, fld.ctypes.data, g, rec.ctypes.data) == -3
    assert np.all(occ == GUARD) and np.all(fld == GUARD * 0x0101) and np.all(rec == GUARD)


# ---- 5. two streams -----------------------------------------------------------------------------------------------------------------------
def loop_context():
    s, cfg = icp_ref.loop_scene(), icp_ref.loop_cfg()
    c = native.Context(0)
    c.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    c.set_materials(params.kaist_materials(), s["object_materials"], 0)
    c.set_config(cfg, icp_ref.LOOP_ANGLES)
    c.set_beam_samples(golden_beams(icp_ref.LOOP_SAMPLES))
    return c, cfg


def test_scoring_on_a_second_stream_beside_a_batch_in_flight(tiles):
    c, rcfg = loop_context()
    A = icp_ref.LOOP_ANGLES
    cfg, fld, scan = score_inputs(0)
    states = some_states(np.random.RandomState(80), 4 * tiles[1] + 5)
    poses = np.stack([icp_ref.loop_pose((0.1 * k, 0.05 * k, 0.01 * k)) for k in range(8)])
    imgs = torch.zeros((8, rcfg.n_cells, A), dtype=torch.uint8, device=DEV)
    n = len(states)
    d_pts, d_cnt, d_st, d_fld = dev(F.points_of(scan)), dev(np.array([len(scan)], np.uint32)), dev(states), dev(fld)
    d_rec = torch.zeros(16 * n, dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()

    def enqueue(stream):
        c.score_poses_device(d_pts.data_ptr(), d_cnt.data_ptr(), len(scan), d_st.data_ptr(), n, d_fld.data_ptr(), cfg, d_rec.data_ptr(), stream)

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
    assert beside == alone == F.score(scan, states, fld, cfg).tobytes()
    imgs.zero_()
    torch.cuda.synchronize()
    c.simulate_batch_device(poses, imgs.data_ptr(), None)
    c.synchronize()
    assert np.array_equal(imgs.cpu().numpy(), busy) and busy.any()   # ... and the batch beside it was not disturbed


# ---- 6. closed loop ---------------------------------------------------------------------------------------------------------------------
def test_closed_loop_a_lattice_search_finds_the_pose_of_a_scan_in_a_map():
    c, _ = loop_context()
    imgs = np.stack([c.simulate(icp_ref.loop_pose(p))[0] for p in (icp_ref.LOOP_A, icp_ref.LOOP_B)])
    pts, offs = c.detect(imgs, icp_ref.LOOP_DET)
    assert len(pts[0]) >= 100 and len(pts[1]) >= 100
    cfg = F.loop_field_cfg()
    occ = c.rasterize_points([pts[0]], offs[:1], cfg, F.loop_map_state())
    assert np.array_equal(occ, F.rasterize([pts[0]], cfg, F.loop_map_state()))
    fld = c.distance_field(occ, cfg)
    assert np.array_equal(fld, F.distance_field(occ, cfg))
    states, xyz = F.loop_lattice()
    rec = c.score_poses(pts[1], states, fld, cfg)
    assert rec.tobytes() == F.score(pts[1], states, fld, cfg).tobytes()          # the GPU's records on its own images: the restatement on those images
    best, centre = int(np.argmin(rec["sum_d2"])), len(states) // 2
    ex, ey, eyaw = F.loop_errors(xyz[best])
    print("closed loop on the GPU: argmin node (%.2f m, %.2f m, %.1f deg) at sum_d2 %d (centre node %d), off the truth by %.3f m, %.3f m, %.3f deg"
          % (xyz[best][0], xyz[best][1], math.degrees(xyz[best][2]), rec["sum_d2"][best], rec["sum_d2"][centre], ex, ey, math.degrees(eyaw)))
    # within the host figure plus one lattice step in each of x, y and yaw: the margin is the lattice's own resolution
    assert ex <= F.LOOP_X_MEASURED + F.LOOP_STEP_XY + 1e-9 and ey <= F.LOOP_Y_MEASURED + F.LOOP_STEP_XY + 1e-9
    assert eyaw <= F.LOOP_YAW_MEASURED + F.LOOP_STEP_YAW + 1e-9
    assert rec["sum_d2"][best] < rec["sum_d2"][centre]                # the argmin beats the centre node A, the identity guess


def test_radar_facade_builds_a_field_and_scores_poses():
    s = icp_ref.loop_scene()
    r = radar.RadarHIP(s["verts"], s["faces"], s["face_object_id"])
    r.loadParams(params.kaist_materials(), s["object_materials"], 0)
    r.updateDynCfg(icp_ref.loop_cfg())
    r.setBeamSamples(golden_beams(icp_ref.LOOP_SAMPLES))
    poses = native.object_poses_array(np.stack([icp_ref.loop_pose(icp_ref.LOOP_A), icp_ref.loop_pose((-1.0, 0.5, math.radians(30.0)))]))
    cfg = F.loop_field_cfg()
    fld = r.buildLikelihoodField(poses, cfg, icp_ref.LOOP_DET)
    assert fld.dtype == np.uint16 and fld.shape == (cfg.height, cfg.width)
    clouds = r.simulatePointClouds(poses, **icp_ref.LOOP_DET)
    keyframes = native.se2_states([0.0, math.radians(30.0)], [0.0, -1.0], [0.0, 0.5])
    want = F.distance_field(F.rasterize(clouds, cfg, radar.RadarHIP._planar_states(poses)), cfg)
    assert np.array_equal(fld, want) and (fld == 0).sum() > 100
    assert np.allclose(radar.RadarHIP._planar_states(poses), keyframes, atol=1e-5)
    states, xyz = F.loop_lattice()
    rec = r.scorePoses(clouds[0], states, fld, cfg)
    assert rec.tobytes() == F.score(clouds[0], states, fld, cfg).tobytes()
    centre = len(states) // 2                                         # a keyframe's own scan sits on the map: nothing scores below it
    assert rec["sum_d2"][centre] == 0 == rec["sum_d2"].min() and rec["n_hit"][centre] == len(clouds[0])
