"""Oriented surface points and point-to-line scan matching on the GPU (rr_surfels.hip) against the numpy restatement of their definition
(tests/surfels_ref.py), byte for byte: every record, count and flag of rr_surface_points at the floor rule, the grid edges, the keep
rule's thresholds, the cap and the overflow bound; the state as raw f64 bits, sse, n_matched, flags and every correspondence of
rr_register_surfels at the edges of the source and target tiling, with ties, truncated, gated-out and degenerate frames and the two-limb
sums at the range limit; the same bytes whatever the order of arrival and on two streams at once; and the closed loop of §22's room, in
which point-to-line must beat point-to-point on the same clouds.  No f64 sqrt or division differed in its last bit on the device: there
is no exception to "byte for byte" here."""
import math

import numpy as np
import pytest

import icp_ref as P
import surfels_ref as R
from common import golden_beams
from radarays_ros_amd import native, params, radar

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
N_ANGLES = 16
GUARD = 0xA5
GATE = 1.5


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    c.set_config(params.kaist_preset(n_cells=64), N_ANGLES)
    return c


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)


def packed(clouds, max_points=None):
    n = len(clouds)
    mp = max(1, max(len(c) for c in clouds)) if max_points is None else max_points
    pts = np.zeros((n, mp), native.POINT_DTYPE)
    offs = np.zeros((n, N_ANGLES + 1), np.uint32)
    for f, c in enumerate(clouds):
        pts[f, :min(len(c), mp)] = P.points_of(np.asarray(c, np.float32).reshape(-1, 2)[:mp])
        offs[f, 1:] = len(c)
    return pts, offs, mp


# ---- surface points -----------------------------------------------------------------------------------------------------------------------
def surfels_device(ctx, clouds, cfg, max_surfels=64, max_points=None, stream=None, short=0):
    """the device form on guarded buffers -> (a list of SURFEL_DTYPE arrays, counts uint32 [n][2])"""
    n = len(clouds)
    pts, offs, mp = packed(clouds, max_points)
    g = native.surfel_config(**cfg)
    need = ctx.surfels_scratch_bytes(n, g)
    d_pts, d_offs = dev(pts), dev(offs)
    d_rec = torch.full((n * max_surfels * 32 + 64,), GUARD, dtype=torch.uint8, device=DEV)
    d_cnt = torch.full((n * 8 + 16,), GUARD, dtype=torch.uint8, device=DEV)
    d_scr = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device=DEV)     # (the scratch's contents before the call do not matter)
    torch.cuda.synchronize()
    ctx.surface_points_device(d_pts.data_ptr(), d_offs.data_ptr(), n, mp, g, d_rec.data_ptr() if max_surfels else None, max_surfels, d_cnt.data_ptr(),
                              d_scr.data_ptr(), need - short, stream)
    torch.cuda.synchronize()
    raw, cnt, scr = d_rec.cpu().numpy(), d_cnt.cpu().numpy(), d_scr.cpu().numpy()
    assert np.all(cnt[n * 8:] == GUARD) and np.all(scr[need:] == 0x5A)  # nothing behind the counts or the scratch
    counts = cnt[:n * 8].view(np.uint32).reshape(n, 2).copy()
    out = []
    for f in range(n):
        k = min(int(counts[f, 0]), max_surfels)
        row = raw[f * max_surfels * 32:(f + 1) * max_surfels * 32]
        assert np.all(row[k * 32:] == GUARD), f                       # nothing past the records that exist
        out.append(row[:k * 32].view(native.SURFEL_DTYPE).copy())
    assert np.all(raw[n * max_surfels * 32:] == GUARD)
    return out, counts


def check_surfels(ctx, clouds, cfg, max_surfels=64, max_points=None):
    got, counts = surfels_device(ctx, clouds, cfg, max_surfels, max_points)
    want, want_counts = R.surface_points([np.asarray(c, np.float32).reshape(-1, 2) for c in clouds], max_surfels=max_surfels, max_points=max_points, **cfg)
    assert np.array_equal(counts, want_counts), (counts, want_counts)
    for f, (a, b) in enumerate(zip(got, want)):
        assert a.tobytes() == b.tobytes(), (f, a, b)
    return got, counts


def wall(x0, y0, x1, y1, m, rs=None, noise=0.0):
    t = np.linspace(0.0, 1.0, m)[:, None]
    p = np.array([x0, y0]) + t * (np.array([x1, y1]) - np.array([x0, y0]))
    if rs is not None:
        p = p + rs.normal(0, noise, p.shape)
    return p.astype(np.float32)


CFG = dict(cell=1.0, width=8, min_points=3, max_ratio=0.25)
S = 1.0 / 256.0


def test_width_one_is_one_cell_and_one_record(ctx):
    cfg = dict(cell=2.0, width=1, min_points=2, max_ratio=1.0)
    got, counts = check_surfels(ctx, [wall(-0.9, 0.5, 0.9, 0.6, 9), wall(-1.5, 0, 1.5, 0, 7), np.zeros((0, 2), np.float32)], cfg)
    assert counts[:, 0].tolist() == [1, 1, 0] and got[0]["count"][0] == 9 and got[1]["count"][0] == 4      # the grid is [-1, 1): x = 1 is outside


def test_cell_borders_and_negative_coordinates_pin_the_floor_rule(ctx):
    # width 8, cell 1 m: the grid spans [-4, 4); points exactly on borders, one quantum below them, and on the outer edges
    pts = np.array([[-1.0, -1.0], [-1.0 - S, -1.0 - S], [-S, -S], [0.0, 0.0], [-4.0, -4.0], [-4.0 - S, 0.5], [4.0 - S, 4.0 - S], [4.0, 0.0],
                    [-0.5, -0.5], [-1.5, -0.25], [-0.25, -1.5], [0.5 * S, -0.5 * S], [-3.5, -3.75], [3.5, 3.25]], np.float32)
    cfg = dict(CFG, min_points=2, max_ratio=1.0)
    got, counts = check_surfels(ctx, [pts, -pts, pts[::-1]], cfg)
    assert counts[0, 0] >= 4 and got[0].tobytes() == got[2].tobytes()
    sums = R.cell_sums(pts, 256, 8)
    assert 3 * 8 + 3 in sums and 2 * 8 + 2 in sums and 4 * 8 + 4 in sums and 0 in sums and 63 in sums      # (-1,-1) floors to cell (3,3), not (4,4)


def test_blocks_clipped_at_every_edge_and_corner(ctx):
    rs = np.random.RandomState(3)
    clouds = []
    for cx, cy in ((-3.5, -3.5), (3.5, -3.5), (-3.5, 3.5), (3.5, 3.5), (0.2, -3.6), (0.2, 3.6), (-3.6, 0.2), (3.6, 0.2)):
        clouds.append(np.concatenate([wall(cx - 0.45, cy - 0.3, cx + 0.45, cy + 0.3, 6, rs, 0.02), wall(-2, -2, 2, 2.5, 9, rs, 0.02)]))
    got, counts = check_surfels(ctx, clouds, dict(CFG, max_ratio=0.5))
    assert np.all(counts[:, 0] >= 2)


def test_min_points_threshold_repeated_point_and_symmetric_square(ctx):
    line = wall(-0.4, 0.3, 0.4, 0.4, 4)
    square = np.array([[0.25, 0.25], [0.75, 0.25], [0.25, 0.75], [0.75, 0.75]], np.float32)
    clouds = [line[:3], line, np.repeat(line[:1], 5, 0), square]
    got, counts = check_surfels(ctx, clouds, dict(CFG, min_points=4, max_ratio=1.0))
    assert counts[:, 0].tolist() == [0, 2, 0, 0]                      # N = min_points - 1, N = min_points, h == 0, d == o == 0


def test_normal_through_the_origin_is_not_negated_and_the_ratio_bounds(ctx):
    radial = wall(0.2, 0.2, 0.8, 0.8, 5)                              # a line through the sensor: n . mean == 0
    blob = np.random.RandomState(5).uniform(0.1, 0.9, (12, 2)).astype(np.float32)
    for ratio, kept in ((0.0, [1, 0]), (1.0, [1, 1])):
        got, counts = check_surfels(ctx, [radial, blob], dict(CFG, max_ratio=ratio))
        assert counts[:, 0].tolist() == kept
    assert got[0]["var_n"][0] == 0.0 and got[0]["nx"][0] < 0 < got[0]["ny"][0]      # (-ty, tx) of the tangent (1, 1) / sqrt 2, as it stands


def test_nan_infinite_and_out_of_range_points_are_skipped_and_an_empty_frame(ctx):
    line = wall(-0.4, 0.3, 0.4, 0.4, 5)
    bad = np.array([[np.nan, 0.1], [0.1, np.inf], [-np.inf, np.nan], [8192.0, 0.0], [0.0, -8192.0], [9000.0, 9000.0], [5.0, 0.0]], np.float32)
    got, counts = check_surfels(ctx, [np.concatenate([bad, line, bad]), bad, np.zeros((0, 2), np.float32)], CFG)
    assert counts[:, 0].tolist() == [2, 0, 0]


def test_the_cap_reports_the_true_count_and_truncation_is_flagged(ctx):
    rs = np.random.RandomState(8)
    cloud = np.concatenate([wall(-3.5, -3, 3.5, -3, 40, rs, 0.01), wall(3, -3.5, 3, 3.5, 40, rs, 0.01)])
    got, counts = check_surfels(ctx, [cloud, cloud[:50]], CFG, max_surfels=5)
    assert counts[0, 0] > 5 and counts[0, 1] == R.SF_CAPPED and len(got[0]) == 5
    got, counts = check_surfels(ctx, [cloud, cloud[:50]], CFG, max_surfels=0)
    assert counts[0, 0] > 5 and len(got[0]) == 0
    got, counts = check_surfels(ctx, [cloud, cloud[:50]], CFG, max_points=50)
    assert counts[:, 1].tolist() == [R.SF_TRUNCATED, 0] and got[0].tobytes() == got[1].tobytes()


def test_cell_q_one_and_4096_at_the_overflow_bound(ctx):
    # cell_q = 4096 (16 m cells): 65,536 points at the far corners of a 3 x 3 block's outer cells -- the shifted coordinates reach
    # -4096 and 8191, N = 2^16, the products their bound of 2^58
    rs = np.random.RandomState(11)
    corner = np.where(rs.randint(0, 2, (65535, 2)) == 0, np.float32(-16.0), np.float32(32.0 - S)).astype(np.float32)
    cloud = np.concatenate([np.array([[0.5, 0.5]], np.float32), corner])
    got, counts = check_surfels(ctx, [cloud], dict(cell=16.0, width=4, min_points=2, max_ratio=1.0), max_surfels=16)
    assert counts[0, 0] >= 1 and got[0]["count"].max() == 65536
    tiny = (np.array([[0, 0], [1, 0], [2, 1], [-1, -1], [-2, -1], [3, 3], [-4, -4], [4, 4]], np.float32) * np.float32(S))
    check_surfels(ctx, [tiny], dict(cell=S, width=8, min_points=2, max_ratio=1.0))


def test_the_same_bytes_twice_permuted_and_in_the_host_form(ctx):
    rs = np.random.RandomState(13)
    chunk = native.surfels_tile_sizes()[1]
    cfg = dict(cell=0.25, width=40, min_points=3, max_ratio=0.2)      # 1,600 cells: more than one chunk of the scan
    assert 40 * 40 > chunk
    clouds = [np.concatenate([wall(-4, -3, 4, -3.2, 300, rs, 0.02), wall(3, -4, 3.3, 4, 300, rs, 0.02)]), wall(-4, 1, 4, 2, 257, rs, 0.03), wall(0, 0, 1, 1, 2)]
    first = check_surfels(ctx, clouds, cfg, max_surfels=256)
    again = surfels_device(ctx, clouds, cfg, max_surfels=256)
    mixed = surfels_device(ctx, [c[rs.permutation(len(c))] for c in clouds][::-1], cfg, max_surfels=256)
    for f in range(3):
        assert first[0][f].tobytes() == again[0][f].tobytes() == mixed[0][2 - f].tobytes()
    assert np.array_equal(first[1], again[1]) and np.array_equal(first[1], mixed[1][::-1]) and first[1][0, 0] > 20
    pts, offs, _ = packed(clouds)
    host, host_counts = ctx.surface_points([pts[f, :len(c)] for f, c in enumerate(clouds)], offs, cfg, 256)
    assert np.array_equal(host_counts, first[1]) and all(a.tobytes() == b.tobytes() for a, b in zip(host, first[0]))
    other = surfels_device(ctx, clouds, cfg, max_surfels=256, stream=torch.cuda.Stream(device=DEV).cuda_stream)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(other[0], first[0]))


def test_surface_points_refusals(ctx):
    with pytest.raises(ValueError, match="scratch"):
        surfels_device(ctx, [wall(0, 0, 1, 1, 4)], CFG, short=1)
    L, g = ctx._L, native.surfel_config(**CFG)
    need = ctx.surfels_scratch_bytes(1, g)
    buf = torch.zeros(need + 4096, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    import ctypes as C
    call = lambda *a: L.rr_surface_points_device(ctx._h, *a)         # noqa: E731
    assert call(p, p, 1, 4, C.byref(g), p, 4, p, p, need - 1, None) == -3 and b"scratch of" in L.rr_last_error(ctx._h)
    for a in ((p, None, 1, 4, C.byref(g), p, 4, p, p, need, None), (p, p, 0, 4, C.byref(g), p, 4, p, p, need, None), (p, p, 1, 65537, C.byref(g), p, 4, p, p, need, None),
              (p, p, 1, 4, None, p, 4, p, p, need, None), (p, p, 1, 4, C.byref(g), None, 4, p, p, need, None), (p, p, 1, 4, C.byref(g), p, 0, p, p, need, None),
              (p, p, 1, 4, C.byref(g), p + 8, 4, p, p, need, None), (p, p, 1, 4, C.byref(g), p, 4, p + 2, p, need, None), (p, p, 1, 4, C.byref(g), p, 4, p, None, need, None),
              (p, p, 1, 4, C.byref(g), p, 4, p, p + 8, need, None), (p, p, 1, 4, C.byref(g), p, -1, p, p, need, None)):
        assert call(*a) == -3, a
    for field, v in (("cell", 0.0), ("cell", 17.0), ("cell", float("nan")), ("width", 0), ("width", 1025), ("min_points", 1), ("min_points", 65537),
                     ("max_ratio", -0.1), ("max_ratio", 1.5), ("max_ratio", float("nan"))):
        bad = native.surfel_config(**CFG)
        setattr(bad, field, v)
        assert call(p, p, 1, 4, C.byref(bad), p, 4, p, p, need, None) == -3 and L.rr_surfels_scratch_bytes(1, C.byref(bad)) == 0, (field, v)
    bad = native.surfel_config(**CFG)
    bad.reserved_[2] = 1
    assert call(p, p, 1, 4, C.byref(bad), p, 4, p, p, need, None) == -3
    assert L.rr_surface_points_device(None, p, p, 1, 4, C.byref(g), p, 4, p, p, need, None) == -1
    bare = native.Context(0)
    assert bare._L.rr_surface_points_device(bare._h, p, p, 1, 4, C.byref(g), p, 4, p, p, need, None) == -2
    assert not buf.cpu().numpy().any()                                # nothing was written


# ---- point-to-line registration -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiles():
    return native.icp_tile_sizes()                                    # both matchers are k_icp_pass: one blocking


def target_surfels(rs, count):
    """surfels on a bent wall: means spread over 30 m, unit normals that turn with the position, so no frame is degenerate"""
    t = rs.uniform(-15, 15, count)
    xy = np.stack([t, 5.0 + 0.02 * t * t + rs.normal(0, 0.3, count)], -1)
    ang = rs.uniform(0, 2 * np.pi, count)
    return R.surfels_of(xy, np.stack([np.cos(ang), np.sin(ang)], -1))


def source_for(rs, tgt, count, yaw=0.02, t=(0.1, -0.1), noise=0.05):
    if count == 0 or len(tgt) == 0:
        return rs.uniform(-10, 10, (count, 2)).astype(np.float32)
    k = rs.randint(0, len(tgt), count)
    q = np.stack([tgt["x"][k], tgt["y"][k]], -1).astype(np.float64) + rs.normal(0, noise, (count, 2)) - np.asarray(t)
    c, s = math.cos(yaw), math.sin(yaw)
    return np.stack([c * q[:, 0] + s * q[:, 1], -s * q[:, 0] + c * q[:, 1]], -1).astype(np.float32)


def register_device(ctx, clouds, tgt, init=None, gate=GATE, iterations=2, max_points=None, max_tgt=None, want_corr=True, stream=None):
    n = len(clouds)
    pts, offs, mp = packed(clouds, max_points)
    mt = max(1, len(tgt)) if max_tgt is None else max_tgt
    t = np.zeros(mt, native.SURFEL_DTYPE)
    t[:min(len(tgt), mt)] = tgt[:mt]
    d_pts, d_offs, d_tgt, d_cnt = dev(pts), dev(offs), dev(t), dev(np.array([len(tgt)], np.uint32))
    d_init = None if init is None else dev(np.ascontiguousarray(init, np.float64))
    d_rec = torch.full((n * 48 + 48,), GUARD, dtype=torch.uint8, device=DEV)
    d_corr = torch.full((n * mp * 4 + 64,), GUARD, dtype=torch.uint8, device=DEV) if want_corr else None
    torch.cuda.synchronize()
    ctx.register_surfels_device(d_pts.data_ptr(), d_offs.data_ptr(), n, mp, d_tgt.data_ptr(), d_cnt.data_ptr(), mt, d_rec.data_ptr(),
                                None if d_init is None else d_init.data_ptr(), gate, iterations, d_corr.data_ptr() if want_corr else None, stream)
    torch.cuda.synchronize()
    rec = d_rec.cpu().numpy()
    assert np.all(rec[n * 48:] == GUARD)
    corr = None
    if want_corr:
        raw = d_corr.cpu().numpy()
        assert np.all(raw[n * mp * 4:] == GUARD)
        corr = raw[:n * mp * 4].view(np.uint32).reshape(n, mp)
    return rec[:n * 48].view(native.ICP_DTYPE).copy(), corr


def same_as_ref(rec, corr, want_rec, want_corr):
    for k in ("c", "s", "tx", "ty"):
        assert np.array_equal(rec[k].view(np.uint64), want_rec[k].view(np.uint64)), (k, rec[k], want_rec[k])
    for k in ("sse", "n_matched", "flags"):
        assert np.array_equal(rec[k], want_rec[k]), (k, rec[k], want_rec[k])
    if corr is not None:
        guard = np.uint32(GUARD * 0x01010101)
        for f, w in enumerate(want_corr):
            assert np.array_equal(corr[f, :len(w)], w), f
            assert np.all(corr[f, len(w):] == guard), f


def check(ctx, clouds, tgt, init=None, gate=GATE, iterations=2, max_points=None, max_tgt=None, **kw):
    rec, corr = register_device(ctx, clouds, tgt, init, gate, iterations, max_points, max_tgt, **kw)
    want_rec, _, want_corr = R.register(clouds, tgt, init, gate, iterations, max_points, max_tgt)
    same_as_ref(rec, corr, want_rec, want_corr)
    return rec, corr


_EDGE = {}


def edge_inputs(tiles, case):
    if case not in _EDGE:
        Sx, T = tiles
        counts, n_tgt = [([0, 1, Sx - 1, 2 * Sx + 1], T + 1), ([Sx, Sx + 1, 65], 2 * T + 1), ([Sx + 1, 3], T - 1), ([Sx - 1, 64], T)][case]
        rs = np.random.RandomState(200 + case)
        tgt = target_surfels(rs, n_tgt)
        clouds = [source_for(rs, tgt, m, yaw=0.01 * (f + 1), t=(0.05 * f, -0.1)) for f, m in enumerate(counts)]
        init = native.se2_states(rs.uniform(-0.02, 0.02, len(counts)), rs.uniform(-0.1, 0.1, len(counts)), rs.uniform(-0.1, 0.1, len(counts)))
        init[:, :2] *= 1.7                                            # not normalised: the call does that
        _EDGE[case] = (clouds, tgt, init)
    return _EDGE[case]


@pytest.mark.parametrize("case", range(4))
def test_tiling_edges_of_source_and_target(ctx, tiles, case):
    clouds, tgt, init = edge_inputs(tiles, case)
    rec, _ = check(ctx, clouds, tgt, init, GATE, 3)
    assert rec["n_matched"].max() > 0


def test_zero_iterations_null_init_and_null_corr(ctx, tiles):
    clouds, tgt, init = edge_inputs(tiles, 2)
    check(ctx, clouds, tgt, init, GATE, 0)
    check(ctx, clouds, tgt, None, GATE, 2)
    rec, corr = check(ctx, clouds, tgt, init, GATE, 2, want_corr=False)
    assert corr is None
    h_rec, h_corr = ctx.register_surfels([P.points_of(c) for c in clouds], packed(clouds)[1], tgt, init, GATE, 2, want_corr=True)
    assert h_rec.tobytes() == rec.tobytes() and all(np.array_equal(a, b) for a, b in zip(h_corr, R.register(clouds, tgt, init, GATE, 2)[2]))


def test_lattice_ties_straddle_a_target_tile_edge(ctx, tiles):
    _, T = tiles
    # targets on an integer lattice, two rows; sources at the midpoints, equally far from two or four of them: ties, also across index T-1 | T
    gx = np.arange(T // 2 + 8, dtype=np.float32)
    xy = np.concatenate([np.stack([gx, np.zeros_like(gx)], -1), np.stack([gx, np.ones_like(gx)], -1)])      # index T // 2 + 8 starts row 1
    order = np.argsort(np.concatenate([2 * np.arange(len(gx)), 2 * np.arange(len(gx)) + 1]), kind="stable")  # interleave the rows: (x, 0), (x, 1), ...
    xy = xy[order]
    ang = np.linspace(0, 3.0, len(xy))
    tgt = R.surfels_of(xy, np.stack([np.cos(ang), np.sin(ang)], -1))
    mid = np.arange(T // 2 - 6, T // 2 + 6, dtype=np.float32)
    src = np.concatenate([np.stack([mid + 0.5, np.full_like(mid, 0.5)], -1), np.stack([mid + 0.5, np.zeros_like(mid)], -1), np.stack([mid, np.full_like(mid, 0.5)], -1)])
    rec, corr = check(ctx, [src.astype(np.float32)], tgt, None, 1.0, 0)
    assert rec["n_matched"][0] == len(src) and (corr[0, :len(src)] < T).any() and (corr[0, :len(src)] >= T).any()


def test_truncated_source_and_target_and_bad_targets(ctx, tiles):
    clouds, tgt, init = edge_inputs(tiles, 2)
    rec, _ = check(ctx, clouds, tgt, init, GATE, 2, max_points=100)
    assert rec["flags"].tolist() == [R.TRUNCATED, 0]
    rec, _ = check(ctx, clouds, tgt, init, GATE, 2, max_tgt=200)
    assert np.all(rec["flags"] & R.TRUNCATED)
    bad = tgt.copy()
    bad["x"][::7], bad["y"][3::7], bad["nx"][5::7], bad["ny"][6::7], bad["x"][1::7] = np.nan, 2048.0, 1.5, np.inf, -3000.0
    check(ctx, clouds, bad, init, GATE, 2)


def test_degenerate_frames_keep_their_state(ctx):
    rs = np.random.RandomState(41)
    tgt = target_surfels(rs, 300)
    far = source_for(rs, tgt, 50) + np.float32(500.0)                 # beyond the gate
    xs = np.linspace(-5, 5, 40).astype(np.float32)
    for normal in ((0.0, 1.0), (1.0, 0.0), (math.sqrt(0.5), math.sqrt(0.5))):       # a corridor: all normals parallel
        corridor = R.surfels_of(np.stack([xs, np.full_like(xs, 2.0)], -1) if normal[0] == 0 else np.stack([np.full_like(xs, 2.0), xs], -1) if normal[1] == 0 else np.stack([xs, 4 - xs], -1),
                                np.tile(np.float32(normal), (40, 1)))
        src = np.stack([corridor["x"] + 0.1, corridor["y"] - 0.2], -1).astype(np.float32)
        init = native.se2_states([0.01], [0.02], [-0.03])
        rec, _ = check(ctx, [src], corridor, init, GATE, 3)
        want = R.normalise(init[0])[0]
        assert rec["flags"][0] == R.DEGENERATE and rec["n_matched"][0] == 40 and (rec["c"][0], rec["s"][0], rec["tx"][0], rec["ty"][0]) == want
    init = native.se2_states([0.3, 0.0], [0.25, 0.0], [-0.5, 0.0])
    rec, corr = check(ctx, [far, source_for(rs, tgt, 50)], tgt, init, GATE, 3)
    assert rec["flags"].tolist() == [R.DEGENERATE, 0] and rec["n_matched"][0] == 0 and rec["sse"][0] == 0 and np.all(corr[0, :50] == R.NONE)
    assert (rec["c"][0], rec["s"][0], rec["tx"][0], rec["ty"][0]) == R.normalise(init[0])[0]


def test_corridors_in_general_directions_are_the_restatements_bytes(ctx):
    """the stated limit (test_surfels_host.py pins what happens): the rounding of the pivots decides, and it decides the same on the device"""
    pairs = [R.corridor(a) for a in R.GENERAL_CORRIDORS]
    for tgt, src in pairs:
        rec, _ = check(ctx, [src], tgt, None, GATE, 3)
        assert rec["flags"][0] == R.DEGENERATE


def test_two_limb_sums_of_65536_pairs_at_the_range_limit(ctx):
    # three surfels at corners of the range square with normals at full scale, 65,536 source points all over the square (4,096 of them on
    # its corners, the fourth included) and a gate that spans it: a coordinate of e reaches 2^18, a0*a0, a0*r and r*r sum past 2^63, sse
    # saturates.  The restatement sums Python ints
    lim = np.float32(2047.9)
    tgt = R.surfels_of([[lim, lim], [-lim, lim], [lim, -lim]], [[1, 1], [-1, 1], [1, -1]])
    rs = np.random.RandomState(43)
    src = (rs.choice([-1.0, 1.0], (65536, 2)) * rs.uniform(1.0, 2047.9, (65536, 2))).astype(np.float32)
    src[:4096] = rs.choice([-1.0, 1.0], (4096, 2)) * np.float32(2047.9)            # the corners themselves
    check(ctx, [src], tgt, None, 8000.0, 1, want_corr=False)          # one solve on the two-limb sums, and a last pass at the state it gave
    rec, _ = check(ctx, [src], tgt, None, 8000.0, 0, want_corr=False)
    assert rec["n_matched"][0] == 65536
    _, (N, H, g, rr, two) = R.line_pass(src[:, 0].copy(), src[:, 1].copy(), tgt, (1.0, 0.0, 0.0, 0.0), np.float32(8000.0) ** 2)
    assert H[0][0] >= 1 << 63 and rr >= 1 << 63 and abs(g[0]) >= 1 << 63      # a single int64 would have overflowed
    assert rec["sse"][0] == 0x7FFFFFFFFFFFFFFF == R.sse_of(two[2])


def test_the_same_bytes_twice_and_with_the_frames_permuted(ctx, tiles):
    clouds, tgt, init = edge_inputs(tiles, 0)
    first = register_device(ctx, clouds, tgt, init, GATE, 5)
    again = register_device(ctx, clouds, tgt, init, GATE, 5)
    assert first[0].tobytes() == again[0].tobytes() and np.array_equal(first[1], again[1])
    perm = [3, 0, 2, 1]
    rec, corr = register_device(ctx, [clouds[k] for k in perm], tgt, init[perm], GATE, 5)
    for at, k in enumerate(perm):
        assert rec[at].tobytes() == first[0][k].tobytes() and np.array_equal(corr[at, :len(clouds[k])], first[1][k, :len(clouds[k])])


def loop_context():
    s, cfg = P.loop_scene(), P.loop_cfg()
    c = native.Context(0)
    c.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    c.set_materials(params.kaist_materials(), s["object_materials"], 0)
    c.set_config(cfg, P.LOOP_ANGLES)
    c.set_beam_samples(golden_beams(P.LOOP_SAMPLES))
    return c, cfg


def test_two_streams_register_different_batches_at_once_beside_a_batch_in_flight(tiles):
    Sx, T = tiles
    c, cfg = loop_context()
    A = P.LOOP_ANGLES
    poses = np.stack([P.loop_pose((0.1 * k, 0.05 * k, 0.01 * k)) for k in range(8)])
    imgs = torch.zeros((8, cfg.n_cells, A), dtype=torch.uint8, device=DEV)
    work = []
    for seed in (31, 32):
        rs = np.random.RandomState(seed)
        tgt = target_surfels(rs, T + 100)
        clouds = [source_for(rs, tgt, m, yaw=0.02) for m in (Sx + 9, 200, 2 * Sx)]
        mp = 2 * Sx
        pts = np.zeros((3, mp), native.POINT_DTYPE)
        offs = np.zeros((3, A + 1), np.uint32)
        for f, cl in enumerate(clouds):
            pts[f, :len(cl)] = P.points_of(cl)
            offs[f, -1] = len(cl)
        b = dict(pts=dev(pts), offs=dev(offs), tgt=dev(tgt), cnt=dev(np.array([len(tgt)], np.uint32)),
                 rec=torch.zeros(3 * 48, dtype=torch.uint8, device=DEV), corr=torch.zeros(3 * mp * 4, dtype=torch.uint8, device=DEV))
        work.append((b, len(tgt), mp, torch.cuda.Stream(device=DEV)))
    torch.cuda.synchronize()

    def enqueue(b, n_tgt, mp, stream):
        p = {k: v.data_ptr() for k, v in b.items()}
        c.register_surfels_device(p["pts"], p["offs"], 3, mp, p["tgt"], p["cnt"], n_tgt, p["rec"], None, GATE, 6, p["corr"], stream)

    def results(b):
        return b["rec"].cpu().numpy().tobytes(), b["corr"].cpu().numpy().tobytes()

    c.simulate_batch_device(poses, imgs.data_ptr(), None)             # a batch in flight on the context's stream
    for b, n_tgt, mp, s in work:
        enqueue(b, n_tgt, mp, s.cuda_stream)
    torch.cuda.synchronize()
    c.synchronize()
    together = [results(b) for b, _, _, _ in work]
    busy = imgs.cpu().numpy().copy()
    for b, n_tgt, mp, _ in work:                                      # one after the other, on the context's stream
        b["rec"].zero_(); b["corr"].zero_()
        torch.cuda.synchronize()
        enqueue(b, n_tgt, mp, None)
        c.synchronize()
    assert [results(b) for b, _, _, _ in work] == together and together[0] != together[1]
    imgs.zero_()
    torch.cuda.synchronize()
    c.simulate_batch_device(poses, imgs.data_ptr(), None)
    c.synchronize()
    assert np.array_equal(imgs.cpu().numpy(), busy) and busy.any()    # ... and the batch beside them was not disturbed


def test_both_matchers_share_one_streams_accumulator_while_it_grows(tiles):
    """point-to-line on 3 frames, point-to-point on 70, point-to-line on 3 again, on one stream with no synchronisation in between: the
    accumulator of that stream grows under calls in flight and holds fourteen words per frame, then eight, then fourteen.  Every byte is
    that of the same call made alone on a fresh context"""
    _, T = tiles
    rs = np.random.RandomState(77)
    surf = target_surfels(rs, T + 1)
    cloud_tgt = np.stack([surf["x"], surf["y"]], -1).astype(np.float32)
    mp = 300
    calls = []
    for line, n in ((True, 3), (False, 70), (True, 3)):
        clouds = [source_for(rs, surf, mp - f % 7, yaw=0.02 + 0.001 * f) for f in range(n)]
        pts, offs, _ = packed(clouds, mp)
        tgt = surf if line else P.points_of(cloud_tgt)
        calls.append((line, n, dict(pts=dev(pts), offs=dev(offs), tgt=dev(tgt), cnt=dev(np.array([len(tgt)], np.uint32)),
                                    rec=torch.zeros(n * 48, dtype=torch.uint8, device=DEV), corr=torch.zeros(n * mp * 4, dtype=torch.uint8, device=DEV))))
    torch.cuda.synchronize()

    def enqueue(c, line, n, b, stream):
        p = {k: v.data_ptr() for k, v in b.items()}
        fn = c.register_surfels_device if line else c.register_points_device
        fn(p["pts"], p["offs"], n, mp, p["tgt"], p["cnt"], T + 1, p["rec"], None, GATE, 2, p["corr"], stream)

    def results(b):
        return b["rec"].cpu().numpy().tobytes(), b["corr"].cpu().numpy().tobytes()

    def fresh():
        c = native.Context(0)
        c.set_config(params.kaist_preset(n_cells=64), N_ANGLES)
        return c

    c, s = fresh(), torch.cuda.Stream(device=DEV)
    for line, n, b in calls:
        enqueue(c, line, n, b, s.cuda_stream)
    torch.cuda.synchronize()
    together = [results(b) for _, _, b in calls]
    alone = []
    for line, n, b in calls:
        b["rec"].zero_(); b["corr"].zero_()
        torch.cuda.synchronize()
        ci = fresh()
        enqueue(ci, line, n, b, s.cuda_stream)
        torch.cuda.synchronize()
        alone.append(results(b))
    assert together == alone
    assert all(any(r[0]) and any(r[1]) for r in alone) and alone[0] != alone[2]


def test_register_refusals(ctx):
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    L = ctx._L
    for a in ((None, p, 2, 4, p, p, 4, None, 1.0, 1, p, None), (p, None, 2, 4, p, p, 4, None, 1.0, 1, p, None), (p, p, 2, 4, None, p, 4, None, 1.0, 1, p, None),
              (p, p, 2, 4, p, None, 4, None, 1.0, 1, p, None), (p, p, 2, 4, p, p, 4, None, 1.0, 1, None, None), (p, p, 0, 4, p, p, 4, None, 1.0, 1, p, None),
              (p, p, 2, 65537, p, p, 4, None, 1.0, 1, p, None), (p, p, 2, 4, p, p, 65537, None, 1.0, 1, p, None), (p, p, 2, 4, p, p, 4, None, 0.0, 1, p, None),
              (p, p, 2, 4, p, p, 4, None, 1.0, 65, p, None), (p, p, 2, 4, p + 8, p, 4, None, 1.0, 1, p, None), (p, p, 2, 4, p, p, 4, p + 4, 1.0, 1, p, None),
              (p, p, 2, 4, p, p, 4, None, 1.0, 1, p + 4, None)):
        assert L.rr_register_surfels_device(ctx._h, *a, None) == -3, a
    assert b"rr_register_surfels_device" in L.rr_last_error(ctx._h)
    bare = native.Context(0)
    assert bare._L.rr_register_surfels_device(bare._h, p, p, 2, 4, p, p, 4, None, 1.0, 1, p, None, None) == -2
    assert not buf.cpu().numpy().any()


# ---- the closed loop of DESIGN.md §22: the room of test_icp_host.py, the same two poses, the GPU's own images ----------------------------
def test_closed_loop_point_to_line_beats_point_to_point_on_the_same_clouds():
    c, cfg = loop_context()
    imgs = np.stack([c.simulate(P.loop_pose(p))[0] for p in (P.LOOP_A, P.LOOP_B)])
    pts, offs = c.detect(imgs, P.LOOP_DET)
    surf, counts = c.surface_points([pts[0]], offs[:1], R.LOOP_SURFELS, 4096)
    want_surf, want_counts = R.surface_points([pts[0]], max_surfels=4096, **R.LOOP_SURFELS)
    assert np.array_equal(counts, want_counts) and surf[0].tobytes() == want_surf[0].tobytes() and len(surf[0]) >= 10
    rec, corr = c.register_surfels([pts[1]], offs[1:], surf[0], None, P.LOOP_GATE, P.LOOP_ITERATIONS, want_corr=True)
    want, _, want_corr = R.register([pts[1]], surf[0], None, P.LOOP_GATE, P.LOOP_ITERATIONS)
    same_as_ref(rec, None, want, None)
    assert np.array_equal(corr[0], want_corr[0])
    p2p = c.register_points([pts[1]], offs[1:], pts[0], None, P.LOOP_GATE, P.LOOP_ITERATIONS)
    yaw_err, t_err = P.loop_errors(rec[0])
    yaw_p2p, t_p2p = P.loop_errors(p2p[0])
    print("closed loop on the GPU, %d surface points: point-to-line yaw error %.4f deg, translation error %.4f m; point-to-point %.4f deg, %.4f m"
          % (len(surf[0]), math.degrees(yaw_err), t_err, math.degrees(yaw_p2p), t_p2p))
    assert rec[0]["flags"] == 0 and yaw_err < yaw_p2p and t_err < t_p2p
    assert yaw_err <= 2 * R.LOOP_YAW_MEASURED and t_err <= 2 * R.LOOP_T_MEASURED     # twice what the restatement measures on the oracle's images


def test_radar_facade_registers_surface_points():
    s = P.loop_scene()
    r = radar.RadarHIP(s["verts"], s["faces"], s["face_object_id"])
    r.loadParams(params.kaist_materials(), s["object_materials"], 0)
    r.updateDynCfg(P.loop_cfg())
    r.setBeamSamples(golden_beams(P.LOOP_SAMPLES))
    pose_a, pose_b = P.loop_pose(P.LOOP_A), P.loop_pose(P.LOOP_B)
    real = r.simulatePointClouds(pose_a[None], **P.LOOP_DET)[0]
    surf, counts = r.surfacePoints(real, R.LOOP_SURFELS)
    assert surf[0].dtype == native.SURFEL_DTYPE and counts[0, 0] == len(surf[0]) >= 10
    rec, fixed = r.registerSurfacePoints(np.stack([pose_b, pose_a]), real, R.LOOP_SURFELS, detect=P.LOOP_DET, gate=P.LOOP_GATE, iterations=P.LOOP_ITERATIONS)
    assert rec.dtype == native.ICP_DTYPE and fixed.shape == (2, 7) and fixed.dtype == np.float32
    cloud_b = r.simulatePointClouds(pose_b[None], **P.LOOP_DET)[0]
    offs = np.zeros((1, 401), np.uint32)
    offs[0, -1] = len(cloud_b)
    assert r.context.register_surfels([cloud_b], offs, surf[0], None, P.LOOP_GATE, P.LOOP_ITERATIONS)[0].tobytes() == rec[0].tobytes()
    want = radar.RadarHIP._corrected_by(np.stack([pose_b, pose_a]), rec)
    assert fixed.tobytes() == want.tobytes() and rec["flags"].tolist() == [0, 0]
