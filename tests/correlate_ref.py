"""Correlative scan matching of include/radarays_mi355.h (rr_field_pyramid, rr_correlate_scan) restated in numpy: f32 where the definition
says f32 (numpy rounds every operation and fuses none), integers everywhere else.  Two searches: `exhaustive`, the argmin over every node
of the window, and `search`, the pruned search with its per-level `evaluated` and `kept` counts, which the GPU tests compare against byte
for byte.  The host tests hold the one to the other, the level-from-level pyramid to a brute-force window minimum, and the look-up to the
true block minimum.  One case list, shared by the host and the GPU tests."""
import numpy as np

import field_ref as F
from radarays_ros_amd import native

CELL_RANGE = 16384.0                      # a point is USABLE iff |u|, |v| < this
MAX_LEVELS = 8


# ---- the anchored cells -------------------------------------------------------------------------------------------------------------
def anchored(points, rot, cfg, max_points=None):
    """one scan under float32 anchor states [n_rot][4] -> (bx, by int64 [n_rot][m], usable bool [n_rot][m]); bx, by are 0 where unusable"""
    x, y = F.xy_of(points)
    if max_points is not None:
        x, y = x[:max_points], y[:max_points]
    st = np.ascontiguousarray(rot, np.float32).reshape(-1, 4)
    px, py = F.move(x[None, :], y[None, :], (st[:, 0:1], st[:, 1:2], st[:, 2:3], st[:, 3:4]))
    cell, x0, y0 = np.float32(cfg.cell), np.float32(cfg.x0), np.float32(cfg.y0)
    with np.errstate(invalid="ignore", over="ignore"):
        u = ((px - x0) / cell).astype(np.float32)
        v = ((py - y0) / cell).astype(np.float32)
        usable = np.isfinite(u) & np.isfinite(v) & (np.abs(u) < np.float32(CELL_RANGE)) & (np.abs(v) < np.float32(CELL_RANGE))
        bx = np.where(usable, np.floor(u), 0).astype(np.int64)
        by = np.where(usable, np.floor(v), 0).astype(np.int64)
    return bx, by, usable


def field_at(field, cfg, x, y):
    """F(x, y): the field inside the grid, cap2 outside; x, y integer arrays"""
    f = np.asarray(field, np.uint16).reshape(cfg.height, cfg.width).astype(np.int64)
    inside = (x >= 0) & (x < cfg.width) & (y >= 0) & (y < cfg.height)
    return np.where(inside, f[np.clip(y, 0, cfg.height - 1), np.clip(x, 0, cfg.width - 1)], cfg.max_dist * cfg.max_dist), inside


# ---- the pyramid ------------------------------------------------------------------------------------------------------------------------
def pyramid(field, cfg, levels):
    """uint16 [levels + 1][height][width], built level from level: four reads at stride 2^(h-1), cap2 beyond the edge"""
    H, W, cap2 = cfg.height, cfg.width, cfg.max_dist * cfg.max_dist
    planes = [np.asarray(field, np.uint16).reshape(H, W).astype(np.int64)]
    for h in range(1, levels + 1):
        s = 1 << (h - 1)
        pad = np.full((H + s, W + s), cap2, np.int64)
        pad[:H, :W] = planes[-1]
        planes.append(np.minimum(np.minimum(pad[:H, :W], pad[:H, s:s + W]), np.minimum(pad[s:s + H, :W], pad[s:s + H, s:s + W])))
    return np.stack(planes).astype(np.uint16)


def pyramid_brute(field, cfg, h, shrink=0):
    """the definition of plane h: the minimum over 0 <= a, b < 2^h of F(x + a, y + b).  shrink = 1 is the BROKEN bound, a window one cell
    too narrow, which the host tests show the cases to catch"""
    H, W, cap2 = cfg.height, cfg.width, cfg.max_dist * cfg.max_dist
    w = max(1, (1 << h) - shrink)
    pad = np.full((H + w, W + w), cap2, np.int64)
    pad[:H, :W] = np.asarray(field, np.uint16).reshape(H, W)
    out = np.full((H, W), cap2, np.int64)
    for b in range(w):
        for a in range(w):
            out = np.minimum(out, pad[b:b + H, a:a + W])
    return out.astype(np.uint16)


def lookup(plane, cfg, h, x, y):
    """Q_h(x, y) for integer arrays: cap2 where the 2^h window misses the grid, else the plane at the clamped corner"""
    span, W, H = 1 << h, cfg.width, cfg.height
    outside = (x >= W) | (y >= H) | (x + span <= 0) | (y + span <= 0)
    p = np.asarray(plane).astype(np.int64)
    return np.where(outside, cfg.max_dist * cfg.max_dist, p[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)])


def block_min(field, cfg, h, x, y):
    """the true minimum of F over the 2^h x 2^h block from (x, y), for integer arrays"""
    out = np.full(np.shape(x), cfg.max_dist * cfg.max_dist, np.int64)
    for b in range(1 << h):
        for a in range(1 << h):
            out = np.minimum(out, field_at(field, cfg, x + a, y + b)[0])
    return out


# ---- scores and bounds ----------------------------------------------------------------------------------------------------------------------
def node_index(r, dx, dy, half_x, half_y):
    return (r * (2 * half_y + 1) + dy + half_y) * (2 * half_x + 1) + dx + half_x


def all_scores(A, field, cfg, half_x, half_y):
    """score(r, dx, dy) of every node -> int64 [n_rot][2*half_y+1][2*half_x+1], a point at a time: the window of the field around its cell"""
    bx, by, usable = A
    H, W, cap2 = cfg.height, cfg.width, cfg.max_dist * cfg.max_dist
    f = np.asarray(field, np.uint16).reshape(H, W).astype(np.int64)
    wx, wy = 2 * half_x + 1, 2 * half_y + 1
    out = np.zeros((bx.shape[0], wy, wx), np.int64)
    for r in range(bx.shape[0]):
        for i in range(bx.shape[1]):
            tile = np.full((wy, wx), cap2, np.int64)
            if usable[r, i]:
                xa, ya = int(bx[r, i]) - half_x, int(by[r, i]) - half_y          # the cell under offset (-half_x, -half_y)
                x0, x1, y0, y1 = max(0, xa), min(W, xa + wx), max(0, ya), min(H, ya + wy)
                if x0 < x1 and y0 < y1:
                    tile[y0 - ya:y1 - ya, x0 - xa:x1 - xa] = f[y0:y1, x0:x1]
            out[r] += tile
    return out


def exhaustive(A, field, cfg, half_x, half_y):
    """the argmin over every node -> (score, node index, rot, dx, dy): the smallest (score, index)"""
    s = all_scores(A, field, cfg, half_x, half_y).reshape(-1)
    k = int(np.argmin(s))                                     # (the first of equal minima: the smallest index)
    wx, wy = 2 * half_x + 1, 2 * half_y + 1
    return int(s[k]), k, k // (wx * wy), k % wx - half_x, (k // wx) % wy - half_y


def bounds(A, planes, cfg, h, r, ox, oy, chunk=2048):
    """LB of the candidates (r, ox, oy) at level h -> int64 [n]: the sum over the points of Q_h(bx + ox, by + oy), cap2 for an unusable point"""
    bx, by, usable = A
    cap2 = cfg.max_dist * cfg.max_dist
    out = np.zeros(len(r), np.int64)
    for a in range(0, len(r), chunk):
        rr = r[a:a + chunk]
        q = lookup(planes[h], cfg, h, bx[rr] + ox[a:a + chunk, None], by[rr] + oy[a:a + chunk, None])
        out[a:a + chunk] = np.where(usable[rr], q, cap2).sum(axis=1)
    return out


def children(r, ox, oy, h, half_x, half_y):
    """the candidates of level h - 1 under the candidates (r, ox, oy) of level h, per parent in the order (oy, ox); those that start beyond
    the window dropped"""
    s = 1 << (h - 1)
    cr = np.repeat(r, 4)
    cx = (ox[:, None] + np.array([0, s, 0, s])).reshape(-1)
    cy = (oy[:, None] + np.array([0, 0, s, s])).reshape(-1)
    keep = (cx <= half_x) & (cy <= half_y)
    return cr[keep], cx[keep], cy[keep]


def search(A, planes, cfg, half_x, half_y, levels, capacity):
    """the pruned search -> one native.CORR_DTYPE record.  `planes` are the pyramid's (a broken pyramid gives a broken search)"""
    n_rot = A[0].shape[0]
    span = 1 << levels
    tx, ty = np.arange(-half_x, half_x + 1, span), np.arange(-half_y, half_y + 1, span)
    r = np.repeat(np.arange(n_rot), len(ty) * len(tx))
    oy = np.tile(np.repeat(ty, len(tx)), n_rot)
    ox = np.tile(tx, n_rot * len(ty))                         # row-major (r, oy, ox)
    lb = bounds(A, planes, cfg, levels, r, ox, oy)
    # 1. the greedy descent: argmin takes the first of equal minima, which is the smallest (r, oy, ox)
    k = int(np.argmin(lb))
    gr, gx, gy, U = r[k:k + 1], ox[k:k + 1], oy[k:k + 1], int(lb[k])
    for h in range(levels, 0, -1):
        cr, cx, cy = children(gr, gx, gy, h, half_x, half_y)
        clb = bounds(A, planes, cfg, h - 1, cr, cx, cy)
        k = int(np.argmin(clb))
        gr, gx, gy, U = cr[k:k + 1], cx[k:k + 1], cy[k:k + 1], int(clb[k])
    rec = np.zeros(1, native.CORR_DTYPE)[0]
    # 2. level-synchronous pruning with that U
    rec["evaluated"][levels] = len(r)
    live = lb <= U
    r, ox, oy, lb = r[live], ox[live], oy[live], lb[live]
    rec["kept"][levels] = len(r)
    overflow = False
    for h in range(levels, 0, -1):
        if len(r) > capacity:
            overflow = True
            break
        r, ox, oy = children(r, ox, oy, h, half_x, half_y)
        lb = bounds(A, planes, cfg, h - 1, r, ox, oy)
        rec["evaluated"][h - 1] = len(r)
        live = lb <= U
        r, ox, oy, lb = r[live], ox[live], oy[live], lb[live]
        rec["kept"][h - 1] = len(r)
    # 3. the winner
    if overflow:
        wr, wdx, wdy = int(gr[0]), int(gx[0]), int(gy[0])
    else:
        # (the greedy node stands among the survivors; named here so that a BROKEN bound, which may prune it, still has a winner)
        r, ox, oy, lb = np.append(r, gr), np.append(ox, gx), np.append(oy, gy), np.append(lb, U)
        key = (lb << 31) | node_index(r, ox, oy, half_x, half_y)
        k = int(np.argmin(key))
        wr, wdx, wdy = int(r[k]), int(ox[k]), int(oy[k])
    bx, by, usable = A
    d, inside = field_at(planes[0], cfg, bx[wr] + wdx, by[wr] + wdy)
    inside = inside & usable[wr]
    d = np.where(inside, d, cfg.max_dist * cfg.max_dist)
    rec["rot"], rec["dx"], rec["dy"], rec["flags"] = wr, wdx, wdy, native.CORR_OVERFLOW if overflow else 0
    rec["sum_d2"], rec["n_in"], rec["n_hit"], rec["upper"] = d.sum(), inside.sum(), (inside & (d <= cfg.gate * cfg.gate)).sum(), U
    return rec


def search_case(c, planes=None, **kw):
    """the restatement's record of a case (with other levels, capacity or planes where given)"""
    levels = kw.get("levels", c["levels"])
    A = anchored(c["points"], c["rot"], c["cfg"], c["max_points"])
    if planes is None:
        planes = pyramid(c["field"], c["cfg"], levels)
    return search(A, planes, c["cfg"], c["half_x"], c["half_y"], levels, kw.get("capacity", c["capacity"]))


def exhaustive_case(c):
    return exhaustive(anchored(c["points"], c["rot"], c["cfg"], c["max_points"]), c["field"], c["cfg"], c["half_x"], c["half_y"])


# ---- the cases the host and the GPU tests share ---------------------------------------------------------------------------------------------
ROOM_W, ROOM_H, ROOM_CELL, ROOM_X0, ROOM_Y0 = 72, 52, 0.25, -10.0, -5.0
ROOM_MAX_DIST, ROOM_GATE = 16, 2


def room_cfg():
    """the grid of the likelihood field's closed loop: 72 x 52 cells of 0.25 m from (-10, -5)"""
    return native.field_config(ROOM_W, ROOM_H, ROOM_CELL, ROOM_X0, ROOM_Y0, ROOM_MAX_DIST, ROOM_GATE)


def room_map():
    """a room's walls, 56 x 36 cells from cell (8, 8), with a door in the south wall and a pillar off centre: no symmetry"""
    occ = np.zeros((ROOM_H, ROOM_W), np.uint8)
    occ[8, 8:64] = occ[43, 8:64] = 1
    occ[8:44, 8] = occ[8:44, 63] = 1
    occ[8, 30:35] = 0
    occ[20:24, 40:46] = 1
    return occ


def wall_scan(occ, cfg, pose, step=3):
    """every step-th occupied cell's centre as the sensor at pose (x, y, yaw) sees it: float32 [m][2] in the sensor frame"""
    iy, ix = np.nonzero(occ)
    qx = cfg.x0 + (ix[::step] + 0.5) * cfg.cell - pose[0]
    qy = cfg.y0 + (iy[::step] + 0.5) * cfg.cell - pose[1]
    c, s = np.cos(pose[2]), np.sin(pose[2])
    return np.stack([c * qx + s * qy, c * qy - s * qx], axis=1).astype(np.float32)


def yaw_states(yaws, x, y):
    return native.se2_states(np.asarray(yaws, np.float64), x, y).astype(np.float32)


ROOM_TRUE = (-2.0 + 5 * ROOM_CELL, -1.0 - 3 * ROOM_CELL, np.radians(2.0))      # the scan's pose: 5 and -3 cells and 2 degrees off the centre
ROOM_CENTRE = (-2.0, -1.0)
ROOM_YAWS = np.radians(np.arange(-4.0, 4.5, 1.0))                               # 9 yaws


def case(label, cfg, field, xy, rot, half_x, half_y, levels, capacity=1 << 12, max_points=None):
    pts = F.points_of(xy)
    return dict(label=label, cfg=cfg, field=np.ascontiguousarray(field, np.uint16), points=pts, rot=np.ascontiguousarray(rot, np.float32),
                half_x=half_x, half_y=half_y, levels=levels, capacity=capacity, max_points=len(pts) if max_points is None else max_points)


def room_case(levels=3, half_x=12, half_y=9, label=None, **kw):
    """the case measured in DESIGN.md: the room, 9 yaws, a window of +-12 x +-9 cells: 4,275 nodes"""
    cfg, occ = room_cfg(), room_map()
    fld = F.distance_field(occ, cfg)
    return case(label or "room L%d %dx%d" % (levels, half_x, half_y), cfg, fld, wall_scan(occ, cfg, ROOM_TRUE),
                yaw_states(ROOM_YAWS, *ROOM_CENTRE), half_x, half_y, levels, **kw)


def wide_case(levels):
    """9 yaws and +-40 cells on the room: 59,049 nodes, most of which throw points off the grid"""
    return room_case(levels, 40, 40, "wide L%d" % levels, capacity=1 << 16)


def random_case(seed):
    rs = np.random.RandomState(seed)
    W, H = int(rs.randint(1, 50)), int(rs.randint(1, 50))
    md = int(rs.choice([1, 3, 9, 40]))
    cfg = native.field_config(W, H, float(rs.choice([0.25, 0.5, 1.0])), float(rs.uniform(-5, 5)), float(rs.uniform(-5, 5)), md, int(rs.randint(0, md + 1)))
    occ = (rs.random_sample((H, W)) < rs.choice([0.0, 0.02, 0.1, 0.5])).astype(np.uint8)
    fld = F.distance_field(occ, cfg)
    m = int(rs.randint(0, 80))
    xy = np.stack([rs.uniform(cfg.x0 - 4, cfg.x0 + W * cfg.cell + 4, m), rs.uniform(cfg.y0 - 4, cfg.y0 + H * cfg.cell + 4, m)], axis=1)
    n_rot = int(rs.randint(1, 5))
    rot = yaw_states(rs.uniform(-0.3, 0.3, n_rot), float(rs.uniform(-2, 2)), float(rs.uniform(-2, 2)))
    return case("random %d" % seed, cfg, fld, xy, rot, int(rs.randint(0, 20)), int(rs.randint(0, 20)), int(rs.randint(0, 6)))


def all_cases():
    out = []
    cfg, occ = room_cfg(), room_map()
    fld = F.distance_field(occ, cfg)
    scan = wall_scan(occ, cfg, ROOM_TRUE, step=1)
    assert len(scan) >= 130
    rot9, rot3, rot1 = yaw_states(ROOM_YAWS, *ROOM_CENTRE), yaw_states(ROOM_YAWS[3:6], *ROOM_CENTRE), yaw_states([np.radians(2.0)], *ROOM_CENTRE)
    # the window 12 x 9, not a multiple of 2^levels, at every level count 0..4
    out += [room_case(levels) for levels in range(5)]
    # point counts at the wave's edges, n_rot 1, 3, 9; max_points below the count
    for m, rot in ((0, rot3), (1, rot1), (63, rot3), (64, rot9), (65, rot1), (130, rot3)):
        out.append(case("count %d rot %d" % (m, len(rot)), cfg, fld, scan[:130:1][:m] if m < 130 else scan[:130], rot, 6, 5, 2))
    out.append(case("max_points 40 of 130", cfg, fld, scan[:130], rot3, 6, 5, 2, max_points=40))
    # windows: half 0, half 1, half_x != half_y, 2^levels larger than the window
    out.append(case("half 0", cfg, fld, scan[:70], rot9, 0, 0, 0))
    out.append(case("half 0 L3", cfg, fld, scan[:70], rot9, 0, 0, 3))
    out.append(case("half 1", cfg, fld, scan[:70], rot3, 1, 1, 1))
    out.append(case("half 17 x 2", cfg, fld, scan[:70], rot3, 17, 2, 3))
    out.append(case("half 2 x 17", cfg, fld, scan[:70], rot3, 2, 17, 3))
    out.append(case("levels 8 over 5 x 3", cfg, fld, scan[:70], rot3, 5, 3, 8))
    # anchors that push the scan off every side of the grid (negative anchored cells, cells beyond the far edges), and a far one: unusable
    for name, (ax, ay) in (("west", (-22.0, -1.0)), ("east", (15.0, -1.0)), ("south", (-2.0, -16.0)), ("north", (-2.0, 14.0)), ("far", (9000.0, -9000.0))):
        out.append(case("anchor " + name, cfg, fld, scan[:100], yaw_states(ROOM_YAWS[3:6], ax, ay), 9, 7, 2))
    # a NaN state among good ones, a NaN and an infinite point among good ones
    bad_rot = rot3.copy()
    bad_rot[1, 2] = np.nan
    out.append(case("nan state", cfg, fld, scan[:100], bad_rot, 9, 7, 2))
    bad_scan = scan[:100].copy()
    bad_scan[7, 0], bad_scan[64, 1], bad_scan[99, 0] = np.nan, np.inf, -1e30
    out.append(case("nan point", cfg, fld, bad_scan, rot3, 9, 7, 2))
    # ties: an empty map (every node ties: index 0 wins, everything survives) ...
    out.append(case("empty map", cfg, F.distance_field(np.zeros_like(occ), cfg), scan[:70], rot3, 6, 5, 2))
    # ... and a mirror-symmetric map under a mirror-symmetric scan: two equal minima, the lower index wins
    sym_cfg = native.field_config(41, 31, 1.0, -20.5, -15.5, 12, 1)
    sym = np.zeros((31, 41), np.uint8)
    sym[10:21, 8] = sym[10:21, 32] = 1                        # two walls, mirror images about the column of cell 20
    wall = np.stack([np.full(11, 0.0), np.arange(-5.0, 6.0)], axis=1)   # one wall's worth of points around the sensor
    out.append(case("mirror", sym_cfg, F.distance_field(sym, sym_cfg), wall, yaw_states([0.0], 0.0, 0.0), 15, 3, 3))
    # the exhaustive search against the pruned one on a wide window
    out += [wide_case(0), wide_case(4)]
    out += [random_case(seed) for seed in range(12)]
    return out
