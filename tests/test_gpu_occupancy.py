"""Occupancy mapping on the GPU (rr_occupancy.hip) against the numpy restatement of its definition (tests/occupancy_ref.py).  The profile, the
hits and the map bit for bit: empty, truncated and fully cut columns, a margin beyond the first bin, max_free_bin at both ends, points on
cell edges, outside every side, NaN and infinite, several points in one cell, the clamp at both ends.  The free pass with ONE scan on grids
at the edges of k_occ_free's blocking, where at most max(1, 1e-3 * cells) cells may differ (the last place of atan2f, the cap of
tests/test_gpu_detect.py for the same function) and each of those must be what the restatement gives one azimuth to the side.  Fusion exact:
n scans in one call are the integer sum of the GPU's own n single-scan calls, in any order and split.  Every refusal with the outputs
untouched; an update on a second stream beside a batch in flight; the host forms; the C++ mirror; and the closed loop of
tests/occupancy_ref.py through the simulator."""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import field_ref as F
import icp_ref
import occupancy_ref as O
from common import golden_beams
from radarays_ros_amd import native, params, radar
from test_gpu_field import GUARD, dev, edge_cloud, guarded, loop_context, payload     # the guarded buffers and the edge cloud of §23's tests

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ANGLES, N_CELLS = 16, 64


def make_ctx(scroll=0):
    c = native.Context(0)
    c.set_config(params.kaist_preset(n_cells=N_CELLS, scroll_image=scroll), N_ANGLES)
    return c, O.polar_of(c._rrcfg)


@pytest.fixture(scope="module")
def ctx():
    return make_ctx()


@pytest.fixture(scope="module")
def tiles():
    return native.occupancy_tile_sizes()


def make_scan(rs, G, empty=(), k_max=3, lo=1):
    """a synthetic scan as rr_detect writes it: up to k_max detections per column, sorted by column then bin; `empty` columns have none"""
    cols, bins = [], []
    for col in range(G.n_angles):
        k = 0 if col in empty else int(rs.randint(1, k_max + 1))
        b = np.sort(rs.choice(np.arange(lo, G.n_cells), k, replace=False))
        cols += [col] * k
        bins += list(b)
    cols, bins = np.asarray(cols, np.int64), np.asarray(bins, np.int64)
    p = np.zeros(len(cols), native.POINT_DTYPE)
    theta = np.float32(G.theta_min) + ((cols - G.scroll) % G.n_angles).astype(np.float32) * np.float32(G.theta_inc)
    r = ((bins.astype(np.float64) + 0.5) * G.resolution).astype(np.float32)
    p["x"], p["y"], p["intensity"], p["column"], p["bin"] = r * np.cos(theta), r * np.sin(theta), 50.0, cols, bins
    offs = np.zeros(G.n_angles + 1, np.uint32)
    offs[1:] = np.cumsum(np.bincount(cols, minlength=G.n_angles))
    return p, offs


def run_update(c, clouds, offs, cfg, m, states=None, max_points=None, evidence=None, stream=None):
    """the device form on guarded buffers -> (evidence int32 [height][width], profile float32 [n][n_angles]).  A cloud longer than
    max_points keeps its true offsets"""
    n = len(clouds)
    mp = max(1, max(len(p) for p in clouds)) if max_points is None else max_points
    pts = np.zeros((n, max(mp, 1)), native.POINT_DTYPE)
    for f, p in enumerate(clouds):
        pts[f, :min(len(p), mp)] = p[:mp]
    cells = cfg.width * cfg.height
    d_ev, d_prof = guarded(4 * cells), guarded(4 * n * N_ANGLES)
    d_ev[:4 * cells] = 0 if evidence is None else dev(np.ascontiguousarray(evidence, np.int32))
    d_pts, d_offs = dev(pts), dev(np.ascontiguousarray(offs, np.uint32).reshape(n, N_ANGLES + 1))
    d_st = None if states is None else dev(np.ascontiguousarray(states, np.float64))
    torch.cuda.synchronize()
    c.occupancy_update_device(d_pts.data_ptr(), d_offs.data_ptr(), n, mp, cfg, O.occ_cfg(m, N_CELLS), d_prof.data_ptr(), d_ev.data_ptr(),
                              None if d_st is None else d_st.data_ptr(), stream)
    torch.cuda.synchronize()
    return (payload(d_ev, 4 * cells).view(np.int32).reshape(cfg.height, cfg.width),
            payload(d_prof, 4 * n * N_ANGLES).view(np.float32).reshape(n, N_ANGLES))


def no_hits(cloud):
    """the same detections with coordinates that are never IN GRID: the update then shows the free pass alone"""
    p = cloud.copy()
    p["x"] = p["y"] = np.nan
    return p


GRID = dict(width=41, height=37, cell=0.2, x0=-4.1, y0=-3.7)           # the sensor range of 64 bins of 0.0595 m (3.8 m) inside it
MODELS = [O.model(3, 0, 0, N_CELLS), O.model(5, 0, 70 - N_CELLS, N_CELLS), O.model(1, 0, N_CELLS, N_CELLS), O.model(127, 0, 2, 0),
          O.model(2, 0, 3, 17)]


# ---- 1. the profile, the hits and the map, bit for bit --------------------------------------------------------------------------------
@pytest.mark.parametrize("scroll", [0, 5])
def test_profile_and_hits_match_the_restatement_bit_for_bit(scroll):
    c, G = make_ctx(scroll)
    cfg = native.field_config(**GRID)
    rs = np.random.RandomState(100 + scroll)
    a, offs_a = make_scan(rs, G, empty=(0, 7, 15), k_max=4)
    b, offs_b = make_scan(rs, G, empty=(), k_max=2, lo=0)
    clouds, offs = [a, b], np.stack([offs_a, offs_b])
    states = np.array([[1.0, 0.0, 0.0, 0.0], [0.6, 0.8, 0.3, -0.2]])
    # max_points cuts a's tail: a column that loses some detections, columns that lose all of them, and columns that keep theirs
    cut = int(offs_a[9]) + 1
    assert offs_a[10] - offs_a[9] >= 1 and len(a) > cut + 3 and len(b) > cut
    for m in MODELS:                                                   # (l_free 0: the evidence is the hits alone)
        for mp in (None, cut, 0):
            ev, prof = run_update(c, clouds, offs, cfg, m, states, mp)
            assert prof.tobytes() == O.profile(clouds, offs, G, m, mp).tobytes(), (m, mp)
            want = m["l_hit"] * O.hit_counts(clouds, cfg, states, mp)
            assert np.array_equal(ev, want), (m, mp)
            if mp is None:
                assert want.sum() == m["l_hit"] * (len(a) + len(b))    # every point is IN GRID here
    full = O.profile(clouds, offs, G, MODELS[0])
    assert np.all(full[0][[(col - G.scroll) % N_ANGLES for col in (0, 7, 15)]] == np.float32(N_CELLS * G.resolution) ** 2)   # empty: free all the way
    cutp = O.profile(clouds, offs, G, MODELS[0], cut)
    assert (cutp[0] == 0).sum() >= 5 and (O.profile(clouds, offs, G, MODELS[0], 0) == 0).sum() == 2 * N_ANGLES - 3
    assert np.all(O.profile(clouds, offs, G, MODELS[2]) [1] == 0) and np.all(O.profile(clouds, offs, G, MODELS[3]) == 0)     # margin past every bin; max_free_bin 0


def test_hits_on_cell_edges_outside_and_on_points_that_are_not_points(ctx):
    c, G = ctx
    cfg = native.field_config(21, 13, 0.3, -2.1, -1.7)
    xy = edge_cloud(cfg)
    xy = np.concatenate([xy, np.repeat(xy[3:4], 5, axis=0)])          # ... and six points in one cell
    rs = np.random.RandomState(7)
    scan, offs = make_scan(rs, G, k_max=6)
    scan = np.resize(scan, len(xy)) if len(scan) < len(xy) else scan[:len(xy)]
    scan["x"], scan["y"] = xy[:, 0], xy[:, 1]
    offs = np.zeros(N_ANGLES + 1, np.uint32)
    offs[1:] = len(scan)                                               # (the hit step reads the total alone)
    m = O.model(7, 0, 0, 0)
    ev, _ = run_update(c, [scan], offs[None], cfg, m)
    want = 7 * O.hit_counts([scan], cfg)
    assert np.array_equal(ev, want) and want.max() >= 6 * 7 and 0 < (want > 0).sum() < len(xy)


def test_the_map_clamps_at_both_ends(ctx):
    c, _ = ctx
    cfg = native.field_config(7, 3, 0.5, 0.0, 0.0)
    ev = np.int32([-2 ** 31, -1000, -129, -128, -127, -1, 0, 1, 126, 127, 128, 1000, 2 ** 31 - 1, 5, -5, 64, -64, 200, -200, 2, 3]).reshape(3, 7)
    d_ev, d_occ = dev(ev), guarded(21)
    torch.cuda.synchronize()
    c.occupancy_map_device(d_ev.data_ptr(), cfg, d_occ.data_ptr())
    torch.cuda.synchronize()
    got = payload(d_occ, 21).reshape(3, 7)
    assert np.array_equal(got, O.to_map(ev)) and got.min() == 0 and got.max() == 255 and got[0, 6] == 128
    assert list(got[0]) == [0, 0, 0, 0, 1, 127, 128] and list(got[1, :5]) == [129, 254, 255, 255, 255]
    assert np.array_equal(c.occupancy_map(ev, cfg), got)               # the host form


# ---- 2. the free pass with ONE scan, at the edges of the blocking ---------------------------------------------------------------------
def free_grids(tiles):
    """(width, height): one cell, an odd small grid (a width that is no multiple of the cells per thread), a workgroup's cell count and one
    to either side of it"""
    group, per_thread, _ = tiles
    assert group == 1024 and per_thread == 4                            # the factorisations below are of 1023, 1024, 1025
    return [(1, 1), (7, 5), (33, 31), (32, 32), (41, 25), (2 * 41 + 1, 25)]


def centre_of(cfg, ix, iy):
    """the f32 centre of a cell: a sensor placed there makes dx = dy = 0 for that cell, atan2f(0, 0)"""
    return (float(np.float32(cfg.x0) + (np.float32(ix) + np.float32(0.5)) * np.float32(cfg.cell)),
            float(np.float32(cfg.y0) + (np.float32(iy) + np.float32(0.5)) * np.float32(cfg.cell)))


@pytest.mark.parametrize("grid", range(6))
def test_free_space_of_one_scan_at_the_edges_of_the_blocking(ctx, tiles, grid):
    c, G = ctx
    W, H = free_grids(tiles)[grid]
    cfg = native.field_config(W, H, 0.15, -0.15 * W / 2, -0.15 * H / 2)
    rs = np.random.RandomState(200 + grid)
    scan, offs = make_scan(rs, G, empty=(3, 4), k_max=2, lo=8)
    scan = no_hits(scan)
    m = O.model(1, 3, 2, N_CELLS - 4)
    on_centre = centre_of(cfg, W // 2, H // 2)
    states = [np.array([[1.0, 0.0, on_centre[0], on_centre[1]]]),                       # the sensor exactly on a cell centre
              native.se2_states([2.3], [0.31], [-0.17]),
              np.array([[0.6 * 1.1, -0.8 * 1.1, -0.4, 0.25]])]                          # not normalised: used as given
    cap = max(1, int(1e-3 * W * H))
    for st in states:
        ev, prof = run_update(c, [scan], offs[None], cfg, m, st)
        free2 = O.profile([scan], offs[None], G, m)
        assert prof.tobytes() == free2.tobytes()
        want, _ = O.free_counts(free2, cfg, G, st)
        assert O.free_counts(free2, cfg, G, st)[0].tobytes() == want.tobytes()          # the restatement against itself: 0
        differ = ev != -3 * want
        print("grid %d x %d, state %s: %d free cells, %d differ (cap %d)" % (W, H, np.round(st[0], 3), int(want.sum()), int(differ.sum()), cap))
        assert differ.sum() <= cap, (W, H, st, int(differ.sum()))
        if differ.any():
            side = [-3 * O.free_counts(free2, cfg, G, st, az_shift=d)[0] for d in (-1, 1)]
            assert np.all((ev[differ] == side[0][differ]) | (ev[differ] == side[1][differ]))
        if W * H > 100:
            assert 0 < want.sum() < W * H                              # free and not free are both there
    ix, iy = W // 2, H // 2                                            # atan2f(0, 0) = 0: azimuth 0, range 0
    ev, _ = run_update(c, [scan], offs[None], cfg, m, states[0])
    assert ev[iy, ix] == (-3 if O.profile([scan], offs[None], G, m)[0, 0] > 0 else 0)


# ---- 3. fusion is exact -------------------------------------------------------------------------------------------------------------------
def fusion_inputs(G, n):
    rs = np.random.RandomState(300 + n)
    scans = [make_scan(rs, G, empty=tuple(rs.choice(N_ANGLES, 2, replace=False)), k_max=3) for _ in range(n)]
    clouds, offs = [s[0] for s in scans], np.stack([s[1] for s in scans])
    states = native.se2_states(rs.uniform(-math.pi, math.pi, n), rs.uniform(-1, 1, n), rs.uniform(-1, 1, n))
    return clouds, offs, states


@pytest.mark.parametrize("n", [1, 2, 17])                              # (rr_occupancy_tile_sizes reports no scan chunk: there is no chunk edge)
def test_an_update_of_n_scans_is_the_sum_of_n_single_scan_updates(ctx, tiles, n):
    c, G = ctx
    assert tiles[2] == 0
    cfg = native.field_config(**GRID)
    m = O.model(5, 2, 3, N_CELLS)
    clouds, offs, states = fusion_inputs(G, n)
    ev, prof = run_update(c, clouds, offs, cfg, m, states)
    singles = [run_update(c, clouds[f:f + 1], offs[f:f + 1], cfg, m, states[f:f + 1]) for f in range(n)]
    assert np.array_equal(ev, np.sum([s[0] for s in singles], axis=0, dtype=np.int64))
    assert prof.tobytes() == np.concatenate([s[1] for s in singles]).tobytes()
    assert (ev > 0).any() and (ev < 0).any()
    if n == 17:                                                        # two calls in either order, and one call: the same bytes
        k = 6
        first = run_update(c, clouds[:k], offs[:k], cfg, m, states[:k])[0]
        ab = run_update(c, clouds[k:], offs[k:], cfg, m, states[k:], evidence=first)[0]
        second = run_update(c, clouds[k:], offs[k:], cfg, m, states[k:])[0]
        ba = run_update(c, clouds[:k], offs[:k], cfg, m, states[:k], evidence=second)[0]
        assert ab.tobytes() == ba.tobytes() == ev.tobytes()
        perm = np.random.RandomState(1).permutation(n)
        assert run_update(c, [clouds[i] for i in perm], offs[perm], cfg, m, states[perm])[0].tobytes() == ev.tobytes()


# ---- 4. refusals: one call per rule, nothing written --------------------------------------------------------------------------------------
def test_refusals_write_nothing(ctx):
    c, _ = ctx
    L, h = c._L, c._h
    d = torch.full((8192,), GUARD, dtype=torch.uint8, device=DEV)
    p = d.data_ptr()
    q, r = p + 2048, p + 4096
    good = native.field_config(8, 8, 0.5, 0.0, 0.0, 4, 2)

    def grid(**kw):
        g = native.RRFieldConfig(good.width, good.height, good.cell, good.x0, good.y0, good.max_dist, good.gate, 0)
        for k, v in kw.items():
            setattr(g, k, v)
        return C.byref(g)

    def occ(**kw):
        o = native.RROccupancyConfig(3, 1, 2, N_CELLS, (C.c_int32 * 4)())
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)

    upd = lambda pts=p, offs=p, n=2, mp=4, st=None, g=None, o=None, prof=q, ev=r: L.rr_occupancy_update_device(   # noqa: E731
        h, pts, offs, n, mp, st, g or grid(), o or occ(), prof, ev, None)
    tomap = lambda ev=p, g=None, out=q: L.rr_occupancy_map_device(h, ev, g or grid(), out, None)                   # noqa: E731
    assert L.rr_occupancy_update_device(None, p, p, 2, 4, None, grid(), occ(), q, r, None) == -1
    assert L.rr_occupancy_map_device(None, p, grid(), q, None) == -1
    bare = native.Context(0)
    assert bare._L.rr_occupancy_update_device(bare._h, p, p, 2, 4, None, grid(), occ(), q, r, None) == -2
    for kw in (dict(pts=None), dict(offs=None), dict(prof=None), dict(ev=None), dict(n=0), dict(n=65536), dict(mp=-1), dict(mp=65537), dict(st=p + 4),
               dict(ev=r + 2), dict(prof=q + 1)):
        assert upd(**kw) == -3 and b"rr_occupancy_update_device" in L.rr_last_error(h), kw
    for kw in (dict(l_hit=0), dict(l_hit=128), dict(l_free=-1), dict(l_free=128), dict(margin_bins=-1), dict(margin_bins=N_CELLS + 1),
               dict(max_free_bin=-1), dict(max_free_bin=N_CELLS + 1)):
        assert upd(o=occ(**kw)) == -3, kw
    for kw in (dict(width=0), dict(width=4097), dict(height=0), dict(height=4097), dict(cell=0.0), dict(cell=-0.5), dict(cell=float("nan")),
               dict(cell=float("inf")), dict(x0=float("nan")), dict(y0=float("-inf"))):
        assert upd(g=grid(**kw)) == -3 and tomap(g=grid(**kw)) == -3, kw
    assert L.rr_occupancy_update_device(h, p, p, 2, 4, None, None, occ(), q, r, None) == -3
    assert L.rr_occupancy_update_device(h, p, p, 2, 4, None, grid(), None, q, r, None) == -3
    for kw in (dict(ev=None), dict(out=None), dict(ev=p + 2)):
        assert tomap(**kw) == -3 and b"rr_occupancy_map_device" in L.rr_last_error(h), kw
    assert L.rr_occupancy_map_device(h, p, None, q, None) == -3
    torch.cuda.synchronize()
    assert bool((d == GUARD).all())
    # max_dist and gate of the grid are ignored: values rr_distance_field refuses pass here (on zeroed buffers: the offsets are read)
    z = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    assert L.rr_occupancy_update_device(h, z.data_ptr(), z.data_ptr(), 2, 4, None, grid(max_dist=0, gate=-7), occ(), z.data_ptr() + 1024,
                                        z.data_ptr() + 2048, None) == 0
    torch.cuda.synchronize()
    # the host forms, on host buffers pre-filled with a pattern
    ev = np.full((8, 8), GUARD * 0x01010101, np.uint32).view(np.int32)
    out = np.full((8, 8), GUARD, np.uint8)
    pts = np.zeros((2, 4), native.POINT_DTYPE)
    offs = np.zeros((2, N_ANGLES + 1), np.uint32)
    for kw in (dict(n=0), dict(n=65536), dict(mp=65537), dict(mp=-1), dict(g=grid(cell=0.0)), dict(o=occ(l_hit=0))):
        a = dict(n=2, mp=4, g=grid(), o=occ())
        a.update(kw)
        assert L.rr_occupancy_update(h, pts.ctypes.data, offs.ctypes.data, a["n"], a["mp"], None, a["g"], a["o"], ev.ctypes.data) == -3, kw
    assert L.rr_occupancy_update(bare._h, pts.ctypes.data, offs.ctypes.data, 2, 4, None, grid(), occ(), ev.ctypes.data) == -2
    assert L.rr_occupancy_map(h, ev.ctypes.data, grid(width=0), out.ctypes.data) == -3 and L.rr_occupancy_map(h, None, grid(), out.ctypes.data) == -3
    assert np.all(ev.view(np.uint32) == GUARD * 0x01010101) and np.all(out == GUARD)


# ---- 5. two streams, 6. the host forms ------------------------------------------------------------------------------------------------
def test_an_update_on_a_second_stream_beside_a_batch_in_flight():
    c, rcfg = loop_context()
    A = icp_ref.LOOP_ANGLES
    G = O.polar_of(c._rrcfg)
    rs = np.random.RandomState(80)
    scans = [make_scan(rs, G, empty=(1,), k_max=2) for _ in range(5)]
    clouds, offs = [s[0] for s in scans], np.stack([s[1] for s in scans])
    states = native.se2_states(rs.uniform(-3, 3, 5), rs.uniform(-2, 2, 5), rs.uniform(-2, 2, 5))
    cfg, m = F.loop_field_cfg(), O.LOOP_MODEL
    mp = max(len(p) for p in clouds)
    pts = np.zeros((5, mp), native.POINT_DTYPE)
    for f, p in enumerate(clouds):
        pts[f, :len(p)] = p
    d_pts, d_offs, d_st = dev(pts), dev(offs), dev(states)
    d_ev = torch.zeros(4 * cfg.width * cfg.height, dtype=torch.uint8, device=DEV)
    d_prof = torch.zeros(4 * 5 * A, dtype=torch.uint8, device=DEV)
    poses = np.stack([icp_ref.loop_pose((0.1 * k, 0.05 * k, 0.01 * k)) for k in range(8)])
    imgs = torch.zeros((8, rcfg.n_cells, A), dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()

    def enqueue(stream):
        c.occupancy_update_device(d_pts.data_ptr(), d_offs.data_ptr(), 5, mp, cfg, O.occ_cfg(m, rcfg.n_cells), d_prof.data_ptr(), d_ev.data_ptr(),
                                  d_st.data_ptr(), stream)

    c.simulate_batch_device(poses, imgs.data_ptr(), None)             # a batch in flight on the context's stream
    enqueue(side.cuda_stream)
    torch.cuda.synchronize()
    c.synchronize()
    beside = d_ev.cpu().numpy().tobytes()
    busy = imgs.cpu().numpy().copy()
    d_ev.zero_()
    torch.cuda.synchronize()
    enqueue(None)                                                    # alone, on the context's stream
    c.synchronize()
    alone = d_ev.cpu().numpy().tobytes()
    assert beside == alone and np.frombuffer(alone, np.int32).any()
    assert d_prof.cpu().numpy().tobytes() == O.profile(clouds, offs, G, m).tobytes()
    imgs.zero_()
    torch.cuda.synchronize()
    c.simulate_batch_device(poses, imgs.data_ptr(), None)
    c.synchronize()
    assert np.array_equal(imgs.cpu().numpy(), busy) and busy.any()   # ... and the batch beside it was not disturbed


def test_the_host_forms_equal_the_device_forms(ctx):
    c, G = ctx
    cfg = native.field_config(**GRID)
    m = O.model(4, 1, 2, N_CELLS - 1)
    clouds, offs, states = fusion_inputs(G, 3)
    want = run_update(c, clouds, offs, cfg, m, states)[0]
    first = c.occupancy_update(clouds[:1], offs[:1], cfg, m, states[:1])
    kept = first.copy()
    both = c.occupancy_update(clouds[1:], offs[1:], cfg, O.occ_cfg(m, N_CELLS), states[1:], evidence=first)
    assert np.array_equal(first, kept) and both.dtype == np.int32
    assert np.array_equal(both, want) and np.array_equal(c.occupancy_update(clouds, offs, cfg, m, states), want)
    assert np.array_equal(c.occupancy_map(want, cfg), O.to_map(want))
    assert np.array_equal(c.occupancy_update(clouds, offs, cfg, m), run_update(c, clouds, offs, cfg, m)[0])       # no states: the identity


# ---- 7. the C++ mirror ------------------------------------------------------------------------------------------------------------------
def test_cpp_build_occupancy_map_equals_the_ctypes_path(tmp_path):
    native.build()
    exe = str(tmp_path / "occupancy_check")
    lib_dir = os.path.join(ROOT, "radarays_ros_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "occupancy_check.cpp"), "-o", exe, "-L", lib_dir, "-lradarays_mi355", "-Wl,-rpath," + lib_dir],
                   check=True)
    A, n_cells, res = 400, 96, 0.0438                                  # the C++ class renders 400 azimuths
    c = native.Context(0)
    c.set_config(params.kaist_preset(n_cells=n_cells, resolution=res, scroll_image=0), A)
    G = O.polar_of(c._rrcfg)
    rs = np.random.RandomState(9)
    scans = [make_scan(rs, G, empty=tuple(range(40, 90)), k_max=2, lo=10) for _ in range(3)]
    clouds, offs = [s[0] for s in scans], np.stack([s[1] for s in scans])
    states = native.se2_states([0.0, 1.0, -2.0], [0.0, 0.5, -0.25], [0.0, -0.5, 1.0])
    cfg, m = native.field_config(60, 50, 0.2, -6.0, -5.0), O.model(3, 2, 4, 90)
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(struct.pack("<8i", n_cells, 3, cfg.width, cfg.height, m["l_hit"], m["l_free"], m["margin_bins"], m["max_free_bin"]))
        f.write(struct.pack("<d3f", res, cfg.cell, cfg.x0, cfg.y0))
        f.write(states.tobytes())
        for p in clouds:
            f.write(struct.pack("<Q", len(p)) + p.tobytes())
    r = subprocess.run([exe, str(inp), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr, r.stdout[-2000:])
    raw = open(out, "rb").read()
    cells = cfg.width * cfg.height
    assert len(raw) == 2 * 5 * cells
    ev = c.occupancy_update(clouds, offs, cfg, m, states)
    mp_ = c.occupancy_map(ev, cfg)
    once = raw[:4 * cells], raw[4 * cells:5 * cells]
    twice = raw[5 * cells:9 * cells], raw[9 * cells:]
    assert once[0] == ev.tobytes() == twice[0] and once[1] == mp_.tobytes() == twice[1]
    assert (ev > 0).any() and (ev < 0).any() and (mp_ == 128).any()


# ---- 8. closed loop ---------------------------------------------------------------------------------------------------------------------
def test_closed_loop_a_phantom_is_a_wall_for_the_rasteriser_and_free_in_the_occupancy_map():
    c, rcfg = loop_context()
    G = O.polar_of(c._rrcfg)
    assert G == O.loop_polar()
    imgs = np.stack([c.simulate(icp_ref.loop_pose(p))[0] for p in O.LOOP_POSES + [icp_ref.LOOP_B]])
    pts, offs = c.detect(imgs, icp_ref.LOOP_DET)
    clean, scan_b = pts[:-1], pts[-1]
    dirty, doffs, phantom = O.inject_phantom(clean, offs[:-1], G)
    cfg, st, m = F.loop_field_cfg(), O.loop_states(), O.LOOP_MODEL
    ev = c.occupancy_update(dirty, doffs, cfg, m, st)
    want = O.update(dirty, doffs, cfg, G, m, st)
    differ = int((ev != want).sum())
    print("closed loop on the GPU: %d cells of %d differ from the restatement on the GPU's images" % (differ, ev.size))
    assert differ <= max(1, int(1e-3 * ev.size) * len(dirty))          # the free pass's cap, once per scan
    occ_map = c.occupancy_map(ev, cfg)
    assert np.array_equal(occ_map, O.to_map(ev))
    occ_raster = c.rasterize_points(dirty, doffs, cfg, st)
    cell, walls = O.loop_checks(occ_raster, occ_map, clean, phantom, cfg, st)      # statements 1 and 2
    fld = c.distance_field(occ_map, cfg, threshold=129)
    states, xyz = F.loop_lattice()
    rec = c.score_poses(scan_b, states, fld, cfg)
    best = int(np.argmin(rec["sum_d2"]))
    print("  phantom cell %s: raster %d, map %d; %d wall cells, the weakest at %d; argmin node (%.2f m, %.2f m, %.1f deg) at sum_d2 %d"
          % (cell, occ_raster[cell], occ_map[cell], int(walls.sum()), int(occ_map[walls].min()), xyz[best][0], xyz[best][1],
             math.degrees(xyz[best][2]), rec["sum_d2"][best]))
    O.loop_argmin_check(xyz[best])                                     # statement 3


def test_radar_facade_builds_an_occupancy_map():
    s = icp_ref.loop_scene()
    r = radar.RadarHIP(s["verts"], s["faces"], s["face_object_id"])
    r.loadParams(params.kaist_materials(), s["object_materials"], 0)
    r.updateDynCfg(icp_ref.loop_cfg())
    r.setBeamSamples(golden_beams(icp_ref.LOOP_SAMPLES))
    poses = native.object_poses_array(np.stack([icp_ref.loop_pose(p) for p in O.LOOP_POSES[:3]]))
    clouds = r.simulatePointClouds(poses, **icp_ref.LOOP_DET)
    st = radar.RadarHIP._planar_states(poses)
    cfg = F.loop_field_cfg()
    ev, occ_map = r.buildOccupancyMap(clouds, st, cfg, l_hit=3, l_free=2)
    assert ev.dtype == np.int32 and occ_map.dtype == np.uint8 and ev.shape == occ_map.shape == (cfg.height, cfg.width)
    assert np.array_equal(occ_map, O.to_map(ev)) and (occ_map > 128).sum() > 50 and (occ_map < 128).sum() > 500
    ev2, _ = r.buildOccupancyMap(clouds[2:], st[2:], cfg, evidence=r.buildOccupancyMap(clouds[:2], st[:2], cfg)[0])
    assert np.array_equal(ev2, ev)
