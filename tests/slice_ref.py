"""Mesh maps of include/radarays_mi355.h (rr_slice_mesh) restated in numpy: the separating-axis predicate in f32 in the header's order of
operations (numpy rounds every operation and fuses none), applied to EVERY cell of the grid -- no candidate box, no tiles, no prefilter.
The GPU tests compare against it byte for byte.  overlap_f64 is the same test in f64 for arbitrary boxes; covering() and tightness() hold
a map -- the restatement's on the CPU, the device's on the GPU -- to the geometry itself with margins that rounding cannot reach; the case
generators are what tests/test_slice_host.py and tests/test_gpu_slice.py both iterate."""
import numpy as np

from radarays_ros_amd import native

F32 = np.float32
OBJECT_NONE = 0xFFFFFFFF
M_CELL, M_Z = 1.0 / 256.0, 1e-4          # the margins of covering and tightness: cells, metres (about 16 f32 ulps at 4096 cells and 64 m)


# ---- the predicate -----------------------------------------------------------------------------------------------------------------------
def _apart2(a, b, r):
    return ((a > r) & (b > r)) | ((a < -r) & (b < -r))


def _sat(u, v, z, cu, cv, cz, hu, hv, hz):
    """no separating axis among the normal and the nine edge axes: corners u, v, z [3] against boxes of centre (cu, cv, cz) and half sides
    (hu, hv, hz), which broadcast.  The dtype is the inputs': every operation is rounded to it.  Edges and normal come from the raw corners;
    the corners are centred on the box first, then the products are formed"""
    with np.errstate(all="ignore"):
        eu = [u[1] - u[0], u[2] - u[1], u[0] - u[2]]
        ev = [v[1] - v[0], v[2] - v[1], v[0] - v[2]]
        ez = [z[1] - z[0], z[2] - z[1], z[0] - z[2]]
        nu = ev[0] * ez[1] - ez[0] * ev[1]
        nv = ez[0] * eu[1] - eu[0] * ez[1]
        nz = eu[0] * ev[1] - ev[0] * eu[1]
        pu, pv, pz = [u[k] - cu for k in range(3)], [v[k] - cv for k in range(3)], [z[k] - cz for k in range(3)]
        d = (nu * pu[0] + nv * pv[0]) + nz * pz[0]
        r = (hu * abs(nu) + hv * abs(nv)) + hz * abs(nz)
        ok = ~((d > r) | (d < -r))
        for j in range(3):
            a, b = j, (j + 2) % 3
            ok &= ~_apart2(ez[j] * pv[a] - ev[j] * pz[a], ez[j] * pv[b] - ev[j] * pz[b], hv * abs(ez[j]) + hz * abs(ev[j]))
            ok &= ~_apart2(eu[j] * pz[a] - ez[j] * pu[a], eu[j] * pz[b] - ez[j] * pu[b], hu * abs(ez[j]) + hz * abs(eu[j]))
            ok &= ~_apart2(ev[j] * pu[a] - eu[j] * pv[a], ev[j] * pu[b] - eu[j] * pv[b], hu * abs(ev[j]) + hv * abs(eu[j]))
        return ok


def cell_coords(tri, cfg, dtype=F32):
    """a posed triangle [3][3] (x, y, z) -> (u [3], v [3], z [3]) under the grid's rule, every operation in `dtype`"""
    t = np.asarray(tri, F32).astype(dtype)
    cell, x0, y0 = dtype(F32(cfg.cell)), dtype(F32(cfg.x0)), dtype(F32(cfg.y0))
    with np.errstate(all="ignore"):
        return (t[:, 0] - x0) / cell, (t[:, 1] - y0) / cell, t[:, 2].copy()


def band(slice_cfg):
    sc = native._slice_cfg(slice_cfg)
    return F32(sc.z_lo), F32(sc.z_hi)


def marks_f32(tri, z_lo, z_hi, cfg):
    """the cells one record marks: bool [height][width]; the header's definition over every cell of the grid"""
    W, H = cfg.width, cfg.height
    none = np.zeros((H, W), bool)
    u, v, z = cell_coords(tri, cfg)
    if not (np.all(np.isfinite(u)) and np.all(np.isfinite(v)) and np.all(np.isfinite(z))):
        return none
    if z.max() < z_lo or z.min() > z_hi:
        return none
    ixf, iyf = np.arange(W, dtype=F32)[None, :], np.arange(H, dtype=F32)[:, None]
    box = ~((u.max() < ixf) | (u.min() > ixf + F32(1))) & ~((v.max() < iyf) | (v.min() > iyf + F32(1)))
    with np.errstate(all="ignore"):
        cz, hz = (z_lo + z_hi) * F32(0.5), (z_hi - z_lo) * F32(0.5)
    return box & _sat(u, v, z, ixf + F32(0.5), iyf + F32(0.5), cz, F32(0.5), F32(0.5), hz)


def slice_mesh(soup_f32, obj, skip, slice_cfg, grid_cfg, occ=None, objects=None):
    """the posed soup float32 [n][3][3], its object ids [n], skip bytes [n_objects] or None, the band and the grid -> (occ uint8
    [height][width], objects uint32 [height][width]): `occ` and `objects` (or an empty grid and a plane of OBJECT_NONE) with every record's
    marks added"""
    g = native._field_cfg(grid_cfg)
    z_lo, z_hi = band(slice_cfg)
    soup = np.asarray(soup_f32, F32).reshape(-1, 3, 3)
    obj = np.asarray(obj, np.uint32).reshape(-1)
    out = np.zeros((g.height, g.width), np.uint8) if occ is None else np.array(occ, np.uint8).reshape(g.height, g.width)
    ids = np.full((g.height, g.width), OBJECT_NONE, np.uint32) if objects is None else np.array(objects, np.uint32).reshape(g.height, g.width)
    for k in range(len(soup)):
        if skip is not None and skip[obj[k]]:
            continue
        m = marks_f32(soup[k], z_lo, z_hi, g)
        out[m] = 1
        ids[m] = np.minimum(ids[m], obj[k])
    return out, ids


def overlap_f64(tri, box):
    """the same separating-axis test in f64: a triangle [3][3] in (u, v, z) against closed boxes (lo [3], hi [3]) whose parts broadcast"""
    t = np.asarray(tri, np.float64)
    u, v, z = t[:, 0], t[:, 1], t[:, 2]
    lo, hi = box
    ok = np.ones(np.broadcast(lo[0], lo[1], lo[2]).shape, bool)
    for k, p in enumerate((u, v, z)):
        ok = ok & ~((p.max() < lo[k]) | (p.min() > hi[k]))
    c = [0.5 * (lo[k] + hi[k]) for k in range(3)]
    h = [0.5 * (hi[k] - lo[k]) for k in range(3)]
    return ok & _sat(u, v, z, c[0], c[1], c[2], h[0], h[1], h[2])


# ---- covering and tightness --------------------------------------------------------------------------------------------------------------
def _bary(n_lattice=16, n_random=200, seed=3):
    k = np.arange(n_lattice + 1)
    a, b = np.meshgrid(k, k, indexing="ij")
    keep = a + b <= n_lattice
    lat = np.stack([a[keep], b[keep], n_lattice - a[keep] - b[keep]], -1) / float(n_lattice)
    rnd = np.random.RandomState(seed).dirichlet((1.0, 1.0, 1.0), n_random)
    return np.concatenate([lat, rnd])


_BARY = _bary()


def live(case):
    """the records of a case that can mark anything: not skipped, every coordinate finite in cell space"""
    g = native._field_cfg(case["grid"])
    for k, tri in enumerate(case["soup"]):
        if case["skip"] is not None and case["skip"][case["obj"][k]]:
            continue
        u, v, z = cell_coords(tri, g, np.float64)
        if np.all(np.isfinite(np.concatenate([u, v, z]))):
            yield np.stack([u, v, z], -1)


def in_range(case):
    """the magnitudes the margins of covering and tightness are worked out for: every coordinate within 4096 cells and 64 m"""
    g = native._field_cfg(case["grid"])
    t = np.array(list(live(case)))
    return len(t) == len(case["soup"]) and bool(np.all(np.abs(t[..., :2]) <= 4096.0) and np.all(np.abs(t[..., 2]) <= 64.0))


def covering(occ, case):
    """every f64 barycentric sample of every live triangle whose z lies at least M_Z inside the band and whose (u, v) lies at least M_CELL
    from every cell border and inside the grid sits in a marked cell.  -> (samples checked, samples in unmarked cells)"""
    g = native._field_cfg(case["grid"])
    z_lo, z_hi = (float(x) for x in band(case["band"]))
    checked = missed = 0
    for t in live(case):
        s = _BARY @ t
        fu, fv = s[:, 0] - np.floor(s[:, 0]), s[:, 1] - np.floor(s[:, 1])
        ok = (s[:, 2] >= z_lo + M_Z) & (s[:, 2] <= z_hi - M_Z) & (fu >= M_CELL) & (fu <= 1 - M_CELL) & (fv >= M_CELL) & (fv <= 1 - M_CELL)
        ok &= (s[:, 0] >= 0) & (s[:, 0] < g.width) & (s[:, 1] >= 0) & (s[:, 1] < g.height)
        ix, iy = np.floor(s[ok, 0]).astype(np.int64), np.floor(s[ok, 1]).astype(np.int64)
        checked += int(ok.sum())
        missed += int((occ[iy, ix] == 0).sum())
    return checked, missed


def tightness(occ, case):
    """every marked cell overlaps some live triangle under overlap_f64 with the cell grown by M_CELL and the band by M_Z.
    -> (marked cells, marked cells that no triangle reaches)"""
    g = native._field_cfg(case["grid"])
    z_lo, z_hi = (float(x) for x in band(case["band"]))
    ix, iy = np.arange(g.width, dtype=np.float64)[None, :], np.arange(g.height, dtype=np.float64)[:, None]
    zero = np.zeros((g.height, g.width))
    lo = (ix - M_CELL + zero, iy - M_CELL + zero, z_lo - M_Z + zero)
    hi = (ix + 1 + M_CELL + zero, iy + 1 + M_CELL + zero, z_hi + M_Z + zero)
    reached = np.zeros((g.height, g.width), bool)
    for t in live(case):
        reached |= overlap_f64(t, (lo, hi))
    marked = occ != 0
    return int(marked.sum()), int((marked & ~reached).sum())


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
def grid(width, height, cell=0.5, x0=-2.0, y0=-1.0):
    return native.field_config(width, height, cell, x0, y0, 8, 0)


def xyz(uvz, cfg):
    """corners given in cell space [..][3] (u, v, z) -> map-frame float32 (x, y, z); exact for a power-of-two cell"""
    p = np.asarray(uvz, np.float64)
    out = p.copy()
    out[..., 0] = cfg.x0 + p[..., 0] * cfg.cell
    out[..., 1] = cfg.y0 + p[..., 1] * cfg.cell
    return out.astype(F32)


def case(label, soup, cfg, z_band=(0.0, 1.0), obj=None, skip=None):
    soup = np.ascontiguousarray(soup, F32).reshape(-1, 3, 3)
    obj = np.zeros(len(soup), np.uint32) if obj is None else np.ascontiguousarray(obj, np.uint32)
    return {"label": label, "soup": soup, "obj": obj, "skip": skip, "band": tuple(float(F32(b)) for b in z_band), "grid": cfg}


def single_cases():
    """one triangle each on a 24 x 20 grid of 0.5 m cells (u and v of a corner are exact), band [0, 1] unless said"""
    g = grid(24, 20)
    up, down = (lambda x: float(np.nextafter(F32(x), F32(np.inf)))), (lambda x: float(np.nextafter(F32(x), F32(-np.inf))))
    flat = lambda z: [[3.25, 4.5, z], [9.75, 6.25, z], [5.5, 11.25, z]]      # noqa: E731
    T = [("wall with no area in xy", [[3.2, 4.1, -1], [7.7, 9.3, -1], [7.7, 9.3, 3]], (0, 1)),
         ("horizontal, inside the band", flat(0.5), (0, 1)),
         ("top exactly on z_lo", [[3.25, 4.5, -1], [9.75, 6.25, 0.0], [5.5, 11.25, -2]], (0, 1)),
         ("bottom exactly on z_hi", [[3.25, 4.5, 1.0], [9.75, 6.25, 2], [5.5, 11.25, 3]], (0, 1)),
         ("horizontal on z_lo", flat(0.0), (0, 1)), ("horizontal on z_hi", flat(1.0), (0, 1)),
         ("one ulp below the band", flat(down(0.25)), (0.25, 1)), ("one ulp above the band", flat(up(1.0)), (0.25, 1)),
         ("top one ulp below z_lo", [[3.25, 4.5, -1], [9.75, 6.25, down(0.25)], [5.5, 11.25, -2]], (0.25, 1)),
         ("oblique through the band", [[2.5, 3.5, -2], [15.25, 6.75, 3], [6.5, 14.25, 0.5]], (0, 1)),
         ("a plane band, oblique", [[2.5, 3.5, -2], [15.25, 6.75, 3], [6.5, 14.25, 0.5]], (0.5, 0.5)),
         ("a plane band, horizontal in it", flat(0.5), (0.5, 0.5)), ("a plane band, horizontal one ulp off", flat(up(0.5)), (0.5, 0.5)),
         ("a vertex on a cell corner", [[5, 5, 0.5], [6.5, 5.5, 0.5], [5.5, 6.5, 0.5]], (0, 1)),
         ("an edge along a cell border", [[4, 3, 0.5], [9, 3, 0.5], [6, 5.5, 0.5]], (0, 1)),
         ("a point inside a cell", [[5.25, 5.25, 0.5]] * 3, (0, 1)), ("a point on a cell corner", [[5, 5, 0.5]] * 3, (0, 1)),
         ("collinear through cell corners", [[2, 2, 0.5], [6, 6, 0.5], [10, 10, 0.5]], (0, 1)),
         ("collinear, oblique", [[2.25, 3.5, 0.2], [6.25, 5.5, 0.5], [10.25, 7.5, 0.8]], (0, 1)),
         ("outside, low u", [[-6, 3, 0.5], [-1.5, 4, 0.5], [-3, 9, 0.5]], (0, 1)), ("outside, high u", [[25.5, 3, 0.5], [30, 4, 0.5], [27, 9, 0.5]], (0, 1)),
         ("outside, low v", [[3, -6, 0.5], [4, -1.5, 0.5], [9, -3, 0.5]], (0, 1)), ("outside, high v", [[3, 21.5, 0.5], [4, 27, 0.5], [9, 23, 0.5]], (0, 1)),
         ("touching the grid's high corner from outside", [[24, 20, 0.5], [27, 21, 0.5], [25, 24, 0.5]], (0, 1)),
         ("across the low u edge", [[-3.5, 6.5, 0.5], [2.5, 4.25, 0.5], [1.5, 9.75, 0.5]], (0, 1)),
         ("across the high u edge", [[21.5, 6.5, 0.5], [27.5, 4.25, 0.5], [22.5, 9.75, 0.5]], (0, 1)),
         ("across the low v edge", [[6.5, -3.5, 0.5], [4.25, 2.5, 0.5], [9.75, 1.5, 0.5]], (0, 1)),
         ("across the high v edge", [[6.5, 17.5, 0.5], [4.25, 23.5, 0.5], [9.75, 18.5, 0.5]], (0, 1)),
         ("across a corner of the grid", [[-2.5, -1.5, 0.2], [3.5, 0.5, 0.5], [0.5, 4.5, 0.9]], (0, 1)),
         ("over the whole grid and beyond", [[-40, -30, 0.5], [90, -20, 0.5], [10, 80, 0.5]], (0, 1))]
    out = [case(("single", name), xyz(t, g), g, b) for name, t, b in T]
    big = F32(1e30)
    far = xyz([[5, 5, 0.5], [6, 7, 0.5], [8, 5, 0.5]], g)
    far[2, 0] = big
    out.append(case(("single", "one corner at 1e30"), far, g))
    out.append(case(("single", "all corners near 1e30"), np.array([[big, 1, 0.5], [big, 2, 0.5], [-big, 1.5, 0.5]], F32), g))
    out.append(case(("single", "z at 1e30"), np.array([[1, 1, -big], [2, 2, big], [3, 1, 0.5]], F32), g))
    return out


def _random_soup(rs, n, cfg, size, z_range=(-1.0, 2.0)):
    """n triangles with corners within `size` cells of a centre in or just around the grid"""
    c = np.stack([rs.uniform(-2, cfg.width + 2, n), rs.uniform(-2, cfg.height + 2, n), rs.uniform(*z_range, n)], -1)
    d = rs.uniform(-1, 1, (n, 3, 3)) * np.array([size, size, 0.6])
    return xyz(c[:, None, :] + d, cfg)


def grid_cases(tile):
    """the degenerate grids, sides at one and two tiles and one to either side, and the odd grid with negative origin and cell 0.3: a dozen
    triangles of mixed sizes, one of them over the whole grid"""
    shapes = [(1, 1), (1, 37), (37, 1), (tile - 1, tile + 1), (tile, tile), (tile + 1, tile - 1), (2 * tile - 1, 2 * tile + 1), (2 * tile, 2 * tile),
              (2 * tile + 1, 2 * tile - 1)]
    out = []
    for k, (W, H) in enumerate(shapes):
        g = grid(W, H)
        rs = np.random.RandomState(100 + k)
        soup = np.concatenate([_random_soup(rs, 6, g, 1.5), _random_soup(rs, 5, g, 0.5 * max(W, H)),
                               xyz([[[-3.5, -2.5, 0.1], [2.0 * W + 3.5, -1.5, 0.6], [-1.5, 2.0 * H + 2.5, 0.9]]], g)])
        out.append(case(("grid", W, H), soup, g, obj=np.arange(len(soup)) % 3))
    g = odd_grid()
    rs = np.random.RandomState(120)
    soup = np.concatenate([_random_soup(rs, 40, g, 2.0), _random_soup(rs, 12, g, 40.0)])
    out.append(case(("grid", g.width, g.height), soup, g, (0.1, 0.9), obj=np.arange(len(soup)) % 5))
    return out


def odd_grid():
    return native.field_config(257, 130, 0.3, -31.7, -12.3, 8, 0)


def boundary_cases(small_cells, n_large_groups):
    """candidate boxes of small_cells - 1, small_cells and small_cells + 1 cells; the thin triangle along the whole diagonal of the odd grid
    and its mirror image, level and tilted through the band; and more long triangles at once than k_slice_large has workgroups"""
    out = []
    g = grid(40, 30)

    def factor(n):
        a = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
        return n // a, a
    for n in (small_cells - 1, small_cells, small_cells + 1):
        nx, ny = factor(n)
        nx, ny = (nx, ny) if nx <= 36 else (36, -(-n // 36))
        t = [[2.25, 3.25, 0.5], [2.25 + nx - 0.5, 3.25 + 0.3 * (ny - 0.5), 0.5], [2.25 + 0.4 * (nx - 0.5), 3.25 + ny - 0.5, 0.5]]
        out.append(case(("box", n, nx * ny), xyz(t, g), g))
    g = odd_grid()
    for name, z in (("level", (0.5, 0.5, 0.5)), ("tilted", (0.38, 0.62, 0.5))):
        a, b = [0.3, 0.2, z[0]], [256.6, 129.7, z[1]]
        for mirror in (False, True):
            p, q = ([a[0], b[1], a[2]], [b[0], a[1], b[2]]) if mirror else (a, b)
            t = [p, q, [q[0] - 0.4, q[1] + (0.7 if not mirror else -0.7), z[2]]]
            out.append(case(("diagonal", name, "mirror" if mirror else "plain"), xyz(t, g), g, (0.45, 0.55)))
    rs = np.random.RandomState(77)
    n = max(300, n_large_groups + 44)
    p = np.stack([rs.uniform(0, 257, n), rs.uniform(0, 130, n), rs.uniform(0.3, 0.5, n)], -1)        # every one of them crosses the band
    q = np.stack([rs.uniform(0, 257, n), rs.uniform(0, 130, n), rs.uniform(0.5, 0.7, n)], -1)
    r = q + np.stack([rs.uniform(-1, 1, n), rs.uniform(-1, 1, n), rs.uniform(-0.1, 0.1, n)], -1)
    out.append(case(("long", n), xyz(np.stack([p, q, r], 1), g), g, (0.45, 0.55), obj=np.arange(n) % 7))
    return out


def count_cases(group_size):
    """1, group - 1, group and group + 1 records, and 4,000 random small triangles"""
    g = grid(64, 48)
    out = []
    for n in (1, group_size - 1, group_size, group_size + 1):
        out.append(case(("records", n), _random_soup(np.random.RandomState(200 + n), n, g, 1.2), g, obj=np.arange(n) % 4))
    out.append(case(("records", 4000), _random_soup(np.random.RandomState(4000), 4000, g, 1.0), g, obj=np.arange(4000) % 9))
    return out


def all_cases(small_cells, tile, group_size, n_large_groups=256):
    return single_cases() + grid_cases(tile) + boundary_cases(small_cells, n_large_groups) + count_cases(group_size)


def box_cells(c):
    """the candidate boxes of a case's live records, in cells each: what decides between the record's own thread and the large list"""
    g = native._field_cfg(c["grid"])
    z_lo, z_hi = band(c["band"])
    out = []
    for tri in c["soup"]:
        u, v, z = cell_coords(tri, g)
        if not np.all(np.isfinite(np.concatenate([u, v, z]))) or z.max() < z_lo or z.min() > z_hi:
            continue
        xlo, xhi = max(np.ceil(u.min()) - 1, 0), min(np.floor(u.max()), g.width - 1)
        ylo, yhi = max(np.ceil(v.min()) - 1, 0), min(np.floor(v.max()), g.height - 1)
        if xlo <= xhi and ylo <= yhi:
            out.append(int(xhi - xlo + 1) * int(yhi - ylo + 1))
    return out


# ---- the closed loop: the box room of tests/icp_ref.py sliced at the sensor's height, a scan taken at pose B scored over field_ref's lattice
LOOP_BAND = (-0.25, 0.25)
# what the restatement gives on the oracle's image (tests/test_slice_host.py measures, prints and pins it): the distance of the best lattice
# node from the truth in x, y (metres) and yaw (radians); the lattice steps are field_ref.LOOP_STEP_XY = 0.25 m and LOOP_STEP_YAW = 1 degree
# the argmin is the node (0.5 m, 0.25 m, 2 degrees), the lattice node nearest the truth, alone at sum_d2 = 62 (the centre node: 171; the map has
# 368 occupied cells)
LOOP_X_MEASURED, LOOP_Y_MEASURED, LOOP_YAW_MEASURED = 0.05, 0.05, 0.0


def loop_soup():
    import icp_ref
    s = icp_ref.loop_scene()
    return np.asarray(s["verts"], F32)[np.asarray(s["faces"]).reshape(-1)].reshape(-1, 3, 3), np.asarray(s["face_object_id"], np.uint32)
