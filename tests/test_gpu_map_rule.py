"""The map calls agree with each other on the rule they share (csrc/rr_pose2d.h, csrc/rr_grid.h): a state rounded to f32 and applied to a
point, and the cell rule.  The per-feature tests hold every call to its own restatement; here ONE reference, field_ref.cells(field_ref.move(...)),
is held against five calls at once on one cloud whose points sit on the rule's edges: cell edges, the grid's borders and one f32 ulp inside
them, -0.0, NaN and infinities, on a grid whose cell coordinates are exact and on one where they are not, under the identity and under a state
whose f64 parts are not f32 values.  Before the GPU is asked anything the numpy restatements are held to that reference on the same inputs."""
import math

import numpy as np
import pytest

import cast_ref
import field_ref as F
import occupancy_ref as O
import refine_ref
from radarays_ros_amd import native, params

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H, MAX_DIST = 5, 3, 4
GRIDS = (dict(cell=0.5, x0=-1.25, y0=0.0), dict(cell=0.3, x0=0.1, y0=0.0))      # u and v exact; u and v inexact
YAW, TX, TY = 0.3, 0.1, -0.05
N_INTERIOR, N_CELLS, RESOLUTION, L_HIT = 14, 64, 0.05, 3


def border(origin, cell, n):
    """the smallest f32 p whose cell coordinate (p - origin) / cell, taken in f32, is >= n: the first coordinate past n cells"""
    origin, cell, n = f32(origin), f32(cell), f32(n)
    p = f32(origin + n * cell)
    while (p - origin) / cell >= n:
        p = np.nextafter(p, f32(-np.inf))
    while not (p - origin) / cell >= n:
        p = np.nextafter(p, f32(np.inf))
    return p


def below(p):
    return np.nextafter(f32(p), f32(-np.inf))


def make_cloud():
    """(POINT_DTYPE cloud, the number of interior points, which lead it).  The interior points lie inside both grids under both states"""
    rs = np.random.RandomState(7)
    xy = [(x, y) for x, y in zip(rs.uniform(0.25, 1.1, N_INTERIOR), rs.uniform(0.12, 0.6, N_INTERIOR))]
    xy += [(-0.75, 0.6), (0.25, 1.0), (-0.9, 0.5), (0.75, 0.5)]                  # on cell edges of the first grid: in x, in y, in both
    for g in GRIDS:
        u0, uw = border(g["x0"], g["cell"], 0), border(g["x0"], g["cell"], W)
        v0, vh = border(g["y0"], g["cell"], 0), border(g["y0"], g["cell"], H)
        assert u0 == f32(g["x0"]) and v0 == f32(g["y0"])
        mx, my = f32(g["x0"]) + f32(1.7) * f32(g["cell"]), f32(g["y0"]) + f32(1.3) * f32(g["cell"])
        xy += [(u0, my), (below(u0), my), (uw, my), (below(uw), my), (mx, vh), (mx, below(vh))]
    xy += [(0.4, v0), (0.4, below(v0))]                                          # v == 0 is the same coordinate on both grids
    for bad in (-0.0, np.nan, np.inf, -np.inf):
        xy += [(bad, 0.4), (0.4, bad)]
    return F.points_of(np.asarray(xy, np.float32)), N_INTERIOR


def reference(cloud, cfg, state):
    x, y = F.xy_of(cloud)
    return F.cells(*F.move(x, y, state), cfg)


def ray_cases(cloud, n_interior, cfg, state):
    """per interior point k: (its bin, the field of a map with only its cell occupied, what the brute-force march of ray k gives there), or
    None for a point that is not IN GRID.  Ray k points at point k and its sample of bin b_k is the point itself, up to rounding"""
    x, y = F.xy_of(cloud)
    bins = 1 + np.arange(n_interior) % 5
    r = cast_ref.bin_range(bins, RESOLUTION)
    dirs = np.stack([x[:n_interior] / r, y[:n_interior] / r], axis=1).astype(np.float32)
    inside, index = reference(cloud, cfg, state)
    beam = native.beam_config(0, N_CELLS, N_CELLS, 1)
    cases = []
    for k in range(n_interior):
        if not inside[k]:
            cases.append(None)
            continue
        occ = np.zeros(W * H, np.uint8)
        occ[index[k]] = 1
        fld = F.distance_field(occ.reshape(H, W), cfg)
        want = int(cast_ref.brute(np.asarray([state], np.float32), dirs, fld, cfg, beam, RESOLUTION)[0, k])
        cases.append((int(bins[k]), fld, want))
    return dirs, beam, cases


@pytest.mark.parametrize("grid", range(len(GRIDS)))
@pytest.mark.parametrize("turned", [False, True])
def test_the_map_calls_share_one_move_and_one_cell_rule(grid, turned):
    cfg = native.field_config(W, H, max_dist=MAX_DIST, gate=MAX_DIST, **GRIDS[grid])
    state64 = native.se2_states(YAW, TX, TY)[0] if turned else np.array([1.0, 0.0, 0.0, 0.0])
    state32 = state64.astype(np.float32)
    if turned:
        assert all(float(f32(v)) != float(v) for v in state64)
        hyp = math.sqrt(state64[0] ** 2 + state64[1] ** 2)                       # the refinement normalises (c, s) in f64: no f32 value moves
        assert f32(state64[0] / hyp) == state32[0] and f32(state64[1] / hyp) == state32[1]
    cloud, n_interior = make_cloud()
    assert 36 <= len(cloud) <= 44
    offs = np.zeros((1, N_INTERIOR + 1), np.uint32)
    offs[0, 1:] = len(cloud)                                                     # every point in image column 0

    inside, index = reference(cloud, cfg, tuple(state64))
    n_in = int(inside.sum())
    counts = np.bincount(index[inside], minlength=W * H).reshape(H, W)
    assert inside[:n_interior].all() and counts.max() >= 2 and not inside[-6:].any()      # (the last six hold a NaN or an infinity)
    if not turned:                                                               # the borders decide as they should
        at = n_interior + 4 + 6 * grid
        assert list(inside[at:at + 6]) == [True, False, False, True, False, True]

    # the restatements alone, before the GPU is held to anything
    G = O.polar(N_CELLS, N_INTERIOR, resolution=RESOLUTION)
    model = O.model(L_HIT, 0, 0, 0)
    full = np.ones((H, W), np.uint8)
    near = refine_ref.nearest_field(full, cfg)
    fld_full = F.distance_field(full, cfg)
    assert np.array_equal(F.rasterize([cloud], cfg, state64[None]) != 0, counts > 0)
    assert np.array_equal(O.update([cloud], offs, cfg, G, model, state64[None]), L_HIT * counts)
    assert F.score(cloud, state32[None], fld_full, cfg)["n_in"][0] == n_in
    assert refine_ref.refine(cloud, state64[None], near, cfg, 0)["n_matched"][0] == n_in
    dirs, beam, cases = ray_cases(cloud, n_interior, cfg, tuple(state32))
    kept = [k for k, c in enumerate(cases) if c is not None and c[2] == c[0]]
    assert 2 * len(kept) >= n_interior, (len(kept), cases)

    c = native.Context(0)
    c.set_config(params.kaist_preset(n_cells=N_CELLS, resolution=RESOLUTION), N_INTERIOR)
    assert np.array_equal(c.rasterize_points([cloud], offs, cfg, state64[None]) != 0, counts > 0)
    assert np.array_equal(c.occupancy_update([cloud], offs, cfg, O.occ_cfg(model, N_CELLS), state64[None]), L_HIT * counts)
    assert c.score_poses(cloud, state32[None], c.distance_field(full, cfg), cfg)["n_in"][0] == n_in
    assert c.refine_poses(cloud, state64[None], c.nearest_field(full, cfg), cfg, 0)["n_matched"][0] == n_in
    for k in kept:
        b, fld, _ = cases[k]
        assert c.cast_map(state32[None], dirs, fld, cfg, beam)[0, k] == b, (k, b)
