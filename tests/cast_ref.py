"""The beam model of include/radarays_mi355.h (rr_scan_profile, rr_cast_map, rr_score_beams) restated in numpy: f32 where the definition says
f32 (numpy rounds every operation and fuses none), integers everywhere else.  `brute` is the DEFINITION, the march over every sampled bin;
`skip_march` is the skip rule exactly as k_cast applies it, ray by ray, and counts its look-ups.  The host tests hold
skip_march to brute element for element; the GPU tests compare the kernels with brute byte for byte.  The point mapping and the cell rule
are field_ref's."""
import math

import numpy as np

import field_ref as F
from radarays_ros_amd import native

f32 = np.float32

# the margins of the skip rule: rr_cast.hip's constants
EPS, SLACK, DIAG, TINY = f32(2.0 ** -22), f32(2.0 ** -8), f32(1.5), f32(2.0 ** -120)
MAX_SKIP, SHRINK, MIN_CELL = f32(65536.0), f32(1.0 - 2.0 ** -10), f32(2.0 ** -64)


def bin_range(b, resolution):
    """rr_polar.h: r = (float)(((double)b + 0.5) * resolution)"""
    return ((np.asarray(b, np.float64) + 0.5) * float(resolution)).astype(np.float32)


def _fields(fields, cfg):
    """one field [height][width] or several [F][height][width] -> int64 [F][height * width]"""
    f = np.asarray(fields, np.uint16)
    return f.reshape(-1, cfg.height * cfg.width).astype(np.int64)


def _which(which, n):
    return np.zeros(n, np.int64) if which is None else np.asarray(which, np.int64).reshape(n)


def brute(states, dirs, fields, cfg, beam, resolution, which=None):
    """the definition.  states float32 [n][4], dirs float32 [A][2], fields uint16 [height][width] (or [F][height][width] with which[n] naming
    the field of every state) -> uint16 [n][A]: per ray the smallest sampled bin that is a hit, bin_end if there is none"""
    st = np.ascontiguousarray(states, np.float32).reshape(-1, 4)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 2)
    flat, wh = _fields(fields, cfg), _which(which, len(st))
    b = np.arange(beam.bin_begin, beam.bin_end, beam.bin_step, dtype=np.int64)
    out = np.full((len(st), len(d)), beam.bin_end, np.int64)
    if len(b) == 0:
        return out.astype(np.uint16)
    r = bin_range(b, resolution)
    with np.errstate(invalid="ignore", over="ignore"):
        x = r[None, :] * d[:, 0:1]                                    # [A][B]
        y = r[None, :] * d[:, 1:2]
    for h in range(len(st)):                                          # (a state at a time keeps the arrays small)
        px, py = F.move(x, y, tuple(st[h]))
        inside, index = F.cells(px, py, cfg)
        hit = inside & (flat[wh[h]][index] == 0)
        any_hit = hit.any(axis=1)
        out[h] = np.where(any_hit, b[np.argmax(hit, axis=1)], beam.bin_end)
    return out.astype(np.uint16)


def skip_march(states, dirs, fields, cfg, beam, resolution, which=None):
    """the skip rule as k_cast applies it -> (uint16 [n][A] as brute, int64 [n][A]: the field look-ups of every ray, int64 [n][A]: the
    samples it computed, IN GRID or not)"""
    st = np.ascontiguousarray(states, np.float32).reshape(-1, 4)
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 2)
    n, A = len(st), len(d)
    flat, wh = _fields(fields, cfg), np.repeat(_which(which, n), A)
    c, s, tx, ty = (np.repeat(st[:, k], A) for k in range(4))
    ca, sa = np.tile(d[:, 0], n), np.tile(d[:, 1], n)
    cell = f32(cfg.cell)
    step_m = abs(f32(float(beam.bin_step) * float(resolution)))
    r_max = abs(f32((float(beam.bin_end) + 0.5) * float(resolution)))
    shrink = SHRINK if cell >= MIN_CELL else f32(0.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        len_cs = np.sqrt((c * c + s * s) + TINY)
        m1, t1 = np.abs(c) + np.abs(s), np.abs(tx) + np.abs(ty)
        len_d = np.sqrt((ca * ca + sa * sa) + TINY)
        inv_g = shrink / (((step_m * len_d) * len_cs) / cell)
        big = (m1 * (np.abs(ca) + np.abs(sa))) * r_max
        err = (EPS * (f32(16.0) * big + t1)) / cell + SLACK
        assert inv_g.dtype == np.float32 and err.dtype == np.float32
        b = np.full(n * A, beam.bin_begin, np.int64)
        e = np.full(n * A, beam.bin_end, np.int64)
        looks, visits = np.zeros(n * A, np.int64), np.zeros(n * A, np.int64)
        live = np.nonzero(b < beam.bin_end)[0]
        while len(live):
            r = bin_range(b[live], resolution)
            x, y = r * ca[live], r * sa[live]
            px = (c[live] * x - s[live] * y) + tx[live]
            py = (s[live] * x + c[live] * y) + ty[live]
            inside, index = F.cells(px, py, cfg)
            d2 = np.where(inside, flat[wh[live], index], 1)
            visits[live] += 1
            looks[live] += inside
            hit = inside & (d2 == 0)
            e[live[hit]] = b[live[hit]]
            q = ((np.floor(np.sqrt(d2.astype(np.float32))) - DIAG) - err[live]) * inv_g[live]
            assert q.dtype == np.float32
            skip = inside & (q >= f32(1.0))                           # (False for a NaN)
            advance = 1 + np.where(skip, np.minimum(np.where(skip, q, f32(0.0)), MAX_SKIP).astype(np.int64), 0)
            b[live] += advance * beam.bin_step
            live = live[~hit & (b[live] < beam.bin_end)]
    return e.reshape(n, A).astype(np.uint16), looks.reshape(n, A), visits.reshape(n, A)


def profile(clouds, offsets, n_cells, n_angles, scroll=0, max_points=None):
    """rr_scan_profile: clouds (n POINT_DTYPE arrays, whole) and offsets uint32 [n][n_angles + 1] -> uint16 [n][n_angles], indexed by
    azimuth a, whose image column is (a + scroll) mod n_angles"""
    offs = np.asarray(offsets, np.uint32).reshape(len(clouds), n_angles + 1).astype(np.int64)
    out = np.full((len(clouds), n_angles), n_cells, np.int64)
    for f, cloud in enumerate(clouds):
        mp = len(cloud) if max_points is None else max_points
        bins = np.asarray(cloud)["bin"].astype(np.int64)
        for a in range(n_angles):
            col = (a + scroll % n_angles) % n_angles
            first, nxt = offs[f, col], offs[f, col + 1]
            if nxt > first and first < mp:
                out[f, a] = min(int(bins[first]), n_cells)
    return out.astype(np.uint16)


def classify(e, first_bin, beam):
    """expected bins [n][A] against ONE profile [A] -> BEAM_DTYPE [n]"""
    e = np.asarray(e).astype(np.int64).reshape(-1, len(first_bin))
    m = np.broadcast_to(np.asarray(first_bin).astype(np.int64)[None, :], e.shape)
    cast = m >= beam.bin_begin
    e_none, m_none = e >= beam.bin_end, m >= beam.bin_end
    both = cast & ~e_none & ~m_none
    d = m - e
    rec = np.zeros(len(e), native.BEAM_DTYPE)
    rec["n_cast"] = cast.sum(axis=1)
    rec["n_none"] = (cast & e_none & m_none).sum(axis=1)
    rec["n_open"] = (cast & e_none & ~m_none).sum(axis=1)
    rec["n_agree"] = (both & (np.abs(d) <= beam.tol_bins)).sum(axis=1)
    rec["n_short"] = (both & (d < -beam.tol_bins)).sum(axis=1)
    rec["n_through"] = (cast & ~e_none & m_none).sum(axis=1) + (both & (d > beam.tol_bins)).sum(axis=1)
    rec["sum_abs"] = np.where(both, np.minimum(np.abs(d), beam.clip_bins), 0).sum(axis=1)
    return rec


def score(first_bin, states, dirs, field, cfg, beam, resolution):
    return classify(brute(states, dirs, field, cfg, beam, resolution), first_bin, beam)


# ---- the cases the host and the GPU tests share --------------------------------------------------------------------------------------------
N_CELLS = 256
SATURATIONS = (1, 2, 16, 255)
BIN_STEPS = (1, 3, 64)
ANGLES = (1, 63, 64, 65, 129, 400)
# (width, height, cell, resolution): the bins of a ray reach across the grid's diagonal; 17, 3 and 0.9 samples per cell
GRIDS = ((8, 8, 0.5, 0.03), (72, 52, 0.25, 0.0875), (257, 130, 0.125, 0.14))
X0, Y0 = -1.5, 2.25


def grid_cfg(k, max_dist):
    W, H, cell, _ = GRIDS[k]
    return native.field_config(W, H, cell, X0, Y0, max_dist, 0)


def map_list(width, height):
    """field_ref's maps (an empty map and a full one among them) and the walls a ray can slip through or graze"""
    H, W = height, width
    maps = dict(F.map_list(W, H))
    iy, ix = np.mgrid[0:H, 0:W]
    maps["diagonal"] = ((ix * H) // W == iy).astype(np.uint8) if W >= H else ((iy * W) // H == ix).astype(np.uint8)      # one cell thick
    if W == H:
        maps["diagonal"] = (ix == iy).astype(np.uint8)               # the rays of a sensor on it graze cell corners
    single = np.zeros((H, W), np.uint8)
    single[H // 3, (2 * W) // 3] = 1
    maps["single"] = single
    ring = np.zeros((H, W), np.uint8)
    ring[0, :] = ring[-1, :] = ring[:, 0] = ring[:, -1] = 1
    maps["ring"] = ring
    maps["checkerboard"] = ((ix + iy) % 2).astype(np.uint8)
    return maps


def dir_table(n_angles, scale=1.0, theta_min=0.1):
    """(cos, sin) of a full turn in n_angles steps, scaled: numpy f64, rounded once to f32 (what native.beam_directions does)"""
    th = theta_min - np.arange(n_angles, dtype=np.float64) * (2.0 * np.pi / n_angles)
    return np.ascontiguousarray((scale * np.stack([np.cos(th), np.sin(th)], axis=1)).astype(np.float32))


def state_list(cfg, occ):
    """float32 [9][4]: the identity rotation at the grid's centre, a sensor inside an occupied cell (where the map has one), a sensor outside
    the grid looking in, a sensor on a cell corner exactly (a power-of-two cell: the coordinates are exact), two non-unit states, a turned
    one, a NaN state and one far away"""
    W, H, cell, x0, y0 = cfg.width, cfg.height, float(cfg.cell), float(cfg.x0), float(cfg.y0)
    cx, cy = x0 + 0.5 * W * cell + 0.013, y0 + 0.5 * H * cell - 0.021
    iy, ix = np.nonzero(occ)
    k = len(iy) // 2
    ox, oy = (x0 + (ix[k] + 0.5) * cell, y0 + (iy[k] + 0.5) * cell) if len(iy) else (cx, cy)
    ex, ey = x0 + (W // 2) * cell, y0 + (H // 2) * cell
    t = math.radians(33.0)
    return np.array([[1.0, 0.0, cx, cy], [1.0, 0.0, ox, oy], [1.0, 0.0, x0 - 3.0 * cell, cy], [1.0, 0.0, ex, ey],
                     [0.5 * math.cos(t), 0.5 * math.sin(t), cx, cy], [0.0, 2.0, cx + cell, cy], [math.cos(2.5), math.sin(2.5), cx - cell, cy + cell],
                     [np.nan, 0.0, cx, cy], [1.0, 0.0, x0 + 1.0e6, cy]], np.float32)


def field_stack(k):
    """every (map, saturation) of grid k -> (names [(map, saturation)], occ uint8 [M][H][W], fields uint16 [M * S][H][W])"""
    W, H = GRIDS[k][:2]
    maps = map_list(W, H)
    names, fields = [], []
    for name, occ in maps.items():
        for md in SATURATIONS:
            names.append((name, md))
            fields.append(F.distance_field(occ, grid_cfg(k, md)))
    return names, maps, np.stack(fields)


def beam(bin_step, n_cells=N_CELLS, bin_begin=0, bin_end=None, tol_bins=0, clip_bins=0):
    return native.beam_config(bin_begin, n_cells if bin_end is None else bin_end, n_cells, bin_step, tol_bins, clip_bins)


# the ONE list of ray cases: tests/test_gpu_cast.py runs every one of them on the GPU against `brute`, tests/test_cast_host.py marches every one
# of them with `skip_march` against `brute`.  A case is a dict: cfg, res, dirs, states, beam and either `field` or (`fields`, `which`)
FULL_ANGLES = 65                                                      # one full lane tile and one lane of the next
WINDOWS = ((0, N_CELLS), (7, 200), (31, 31))
AZIMUTH_GRID = 1
AZIMUTH_MAPS = ((1.0, "diagonal", 16), (1.0, "ring", 255), (0.5, "random1", 2), (2.0, "checkerboard", 1), (1.0, "single", 16))


def full_cases(k):
    """grid k: every map x saturation x bin step at FULL_ANGLES azimuths, the whole range as the window -> (names, per-name states, cases);
    a case holds the states of all (map, saturation) at once, `which` naming each state's field"""
    res = GRIDS[k][3]
    names, maps, fields = field_stack(k)
    cfg = grid_cfg(k, 16)
    sts = [state_list(cfg, maps[name]) for name, _ in names]
    which = np.repeat(np.arange(len(names)), [len(s) for s in sts])
    dirs = dir_table(FULL_ANGLES)
    cases = [dict(cfg=cfg, res=res, dirs=dirs, states=np.concatenate(sts), fields=fields, which=which, beam=beam(step), step=step) for step in BIN_STEPS]
    return names, sts, cases


def azimuth_cases(A):
    """A azimuths on grid AZIMUTH_GRID: five maps with direction tables of norm 1, 0.5 and 2, every bin step, every window"""
    k = AZIMUTH_GRID
    res = GRIDS[k][3]
    maps = map_list(*GRIDS[k][:2])
    for scale, name, md in AZIMUTH_MAPS:
        cfg = grid_cfg(k, md)
        fld = F.distance_field(maps[name], cfg)
        dirs, sts = dir_table(A, scale), state_list(cfg, maps[name])
        for step in BIN_STEPS:
            for begin, end in WINDOWS:
                yield dict(cfg=cfg, res=res, dirs=dirs, states=sts, field=fld, beam=beam(step, bin_begin=begin, bin_end=end),
                           label=(A, name, md, scale, step, begin, end))


def ring_field(md=16):
    k = AZIMUTH_GRID
    cfg = grid_cfg(k, md)
    occ = map_list(*GRIDS[k][:2])["ring"]
    return cfg, occ, F.distance_field(occ, cfg), GRIDS[k][3]


RECORD_ANGLES, RECORD_TOL = 129, 5


def records_case(per_wave, per_group):
    """the records test: a pool of 309 states around the centre of the ring map, hypothesis counts at the edges of a wave's and a workgroup's
    tile, a window that begins late and ends early, and one with bin_begin == bin_end"""
    A, tol = RECORD_ANGLES, RECORD_TOL
    cfg, occ, fld, res = ring_field()
    rs = np.random.RandomState(27)
    base = state_list(cfg, occ)
    pool = np.concatenate([base, base[:1] + np.concatenate([np.zeros((300, 2)), rs.uniform(-4.0, 4.0, (300, 2))], axis=1).astype(np.float32)])
    counts = sorted({1, per_wave - 1, per_wave, per_wave + 1, per_group - 1, per_group, per_group + 1, 257} - {0})
    return dict(cfg=cfg, res=res, dirs=dir_table(A), states=pool, field=fld, beam=beam(1, bin_begin=10, bin_end=240, tol_bins=tol, clip_bins=9),
                empty_beam=beam(1, bin_begin=31, bin_end=31, tol_bins=3, clip_bins=3), counts=counts, rs=rs)


def small_case(A=FULL_ANGLES):
    """the host-form test: the ring map, bin step 3, a window inside the range, a random profile"""
    cfg, occ, fld, res = ring_field()
    rs = np.random.RandomState(5)
    return dict(cfg=cfg, res=res, dirs=dir_table(A), states=state_list(cfg, occ), field=fld, first=rs.randint(0, N_CELLS + 1, A).astype(np.uint16),
                beam=beam(3, bin_begin=2, bin_end=250, tol_bins=4, clip_bins=16))


def stream_case():
    """the two-stream test, under the closed loop's polar config (64 azimuths, 320 bins): 69 states around the centre of the ring map"""
    import icp_ref
    rcfg = icp_ref.loop_cfg()
    cfg, occ, fld, _ = ring_field()
    rs = np.random.RandomState(81)
    base = state_list(cfg, occ)[:1]
    states = (base + np.concatenate([np.zeros((69, 2)), rs.uniform(-3.0, 3.0, (69, 2))], axis=1)).astype(np.float32)
    first = rs.randint(0, 300, icp_ref.LOOP_ANGLES).astype(np.uint16)
    return dict(cfg=cfg, res=float(rcfg.resolution), dirs=native.beam_directions(native.make_config(rcfg, icp_ref.LOOP_ANGLES)), states=states,
                field=fld, first=first, beam=native.beam_config(0, 300, rcfg.n_cells, 1, 4, 16))


def host_cases(per_wave, per_group):
    """every ray case of the GPU tests that needs no GPU to state: what tests/test_cast_host.py marches.  (The closed loop and the façade run on
    the GPU's own images; their host counterpart is the closed loop on the oracle's images.)"""
    for k in range(len(GRIDS)):
        for c in full_cases(k)[2]:
            yield dict(c, label=("full", k, c["step"]))
    for A in ANGLES:
        if A != FULL_ANGLES:
            yield from azimuth_cases(A)
    r = records_case(per_wave, per_group)
    yield dict(r, label=("records",))
    yield dict(r, beam=r["empty_beam"], label=("records, empty window",))
    yield dict(small_case(), label=("host forms",))
    yield dict(stream_case(), label=("two streams",))


def case_fields(c):
    return (c["fields"], c["which"]) if "fields" in c else (c["field"], None)


def case_brute(c):
    f, w = case_fields(c)
    return brute(c["states"], c["dirs"], f, c["cfg"], c["beam"], c["res"], w)


def case_skip(c):
    f, w = case_fields(c)
    return skip_march(c["states"], c["dirs"], f, c["cfg"], c["beam"], c["res"], w)


# ---- the closed loop of the host and GPU tests: §24's room, eight poses, grid and occupancy model (tests/occupancy_ref.py); the field is the
# occupancy map's at threshold 129.  The window runs from the detector's min_bin to the bin of the room's diagonal; tol_bins is the bins in one
# cell's diagonal, rounded up: 0.25 m * sqrt(2) / 0.0595 m = 5.94 -> 6; clip_bins = 4 * tol_bins
LOOP_MAX_DIST = 16
LOOP_THRESHOLD = 129


def loop_beam(resolution, cell=F.LOOP_CELL, min_bin=0):
    import icp_ref
    diag = math.hypot(icp_ref.LOOP_HI[0] - icp_ref.LOOP_LO[0], icp_ref.LOOP_HI[1] - icp_ref.LOOP_LO[1])
    tol = int(math.ceil(cell * math.sqrt(2.0) / resolution))
    return native.beam_config(min_bin, min(int(diag / resolution), icp_ref.LOOP_CELLS), icp_ref.LOOP_CELLS, 1, tol, 4 * tol)


def loop_behind_wall():
    """a state moved from A straight through the nearest wall, by that wall's distance plus 1 m -> float32 [2][4]: A itself, and that state"""
    import icp_ref
    ax, ay, yaw = icp_ref.LOOP_A
    walls = [(ax - icp_ref.LOOP_LO[0], (-1.0, 0.0)), (icp_ref.LOOP_HI[0] - ax, (1.0, 0.0)), (ay - icp_ref.LOOP_LO[1], (0.0, -1.0)),
             (icp_ref.LOOP_HI[1] - ay, (0.0, 1.0))]
    dist, (ux, uy) = min(walls)
    return native.se2_states([yaw, yaw], [ax, ax + (dist + 1.0) * ux], [ay, ay + (dist + 1.0) * uy]).astype(np.float32)


def loop_best(recs):
    """the node with the most n_agree, ties broken by the smaller sum_abs (then by the lower index)"""
    return int(np.lexsort((np.arange(len(recs)), recs["sum_abs"], -recs["n_agree"].astype(np.int64)))[0])


def loop_check(recs, xyz, recs_wall):
    """the two statements of the closed loop -> the argmax node's index"""
    best = loop_best(recs)
    ex, ey, eyaw = F.loop_errors(xyz[best])
    assert ex <= F.LOOP_STEP_XY + 1e-9 and ey <= F.LOOP_STEP_XY + 1e-9 and eyaw <= F.LOOP_STEP_YAW + 1e-9, (tuple(xyz[best]), recs[best])
    assert recs_wall[1]["n_through"] > recs_wall[0]["n_through"], recs_wall
    return best
