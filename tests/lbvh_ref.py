"""Plain helpers of the tree-builder edge tests (tests/test_lbvh_host.py, tests/test_gpu_lbvh_edges.py): small scenes that sit
on the structural decisions of rr_lbvh.hip, the seeded rays that probe them, the brute-force side, and k_split / clip_tri_box /
k_prim of rr_lbvh.hip restated in numpy f32 (the library is built without FMA contraction, so every operation rounds as here).

Nothing here needs a GPU.  The reference of a case is the oracle's brute-force loop over its triangles; it is computed once per
case and process (case()) and shared, unchanged, by every test that asks for it."""
import numpy as np

import dynamic_ref as R

f32 = np.float32
K_MAX_CELLS = 24                 # kMaxCellsPerAxis
K_MAX_LEAF = 4                   # kMaxLeafTris
COUNTS = (2, 3, 4, 5, 8, 9, 255, 256, 257, 513)
FAR_OFFSET = np.array([6000.0, -6000.0, 500.0])
LATTICE_K = tuple(range(4, 17))
AIMED_PER_HUGE, LATTICE_PER_K = 150, 6


def _soup(tris):
    v = np.ascontiguousarray(np.asarray(tris, np.float64).reshape(-1, 3), np.float32)
    return v, np.arange(len(v), dtype=np.uint32).reshape(-1, 3)


def _rotations(rs, n):
    q = rs.normal(0, 1, (n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(n, 3, 3)


_UNIT = np.array([[0.5, 0.0, 0.0], [-0.25, 0.4330127, 0.0], [-0.25, -0.4330127, 0.0]])        # edge 0.87 m, centroid at 0


# ---- the scenes -------------------------------------------------------------------------------------------------------
def separated(n):
    """1. n congruent triangles, each turned its own way, on a 4 m grid: no face is larger than another"""
    rs = np.random.RandomState(7000 + n)
    m = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
    cell = np.stack(np.unravel_index(rs.permutation(m ** 3)[:n], (m, m, m)), -1) * 4.0
    tri = np.einsum("nij,kj->nki", _rotations(rs, n), _UNIT) + cell[:, None, :]
    return _soup(tri)


def coincident():
    """2. 300 triangles of 0.06 .. 8 m whose BOXES share one centre exactly, then 150 pairs that share theirs.  Every
    coordinate is a multiple of 2^-9 below 64 m, so the shifts are exact in f32 and the box centres are equal bit for bit."""
    rs = np.random.RandomState(7100)
    g = 2.0 ** -9

    def centred(size, centre):
        t = np.round(rs.normal(0, 1, (3, 3)) * size / (2 * g)) * (2 * g)
        while np.linalg.norm(np.cross(t[1] - t[0], t[2] - t[0])) < 1e-6:
            t = np.round(rs.normal(0, 1, (3, 3)) * size / (2 * g)) * (2 * g)
        return t - 0.5 * (t.min(0) + t.max(0)) + centre

    tris = [centred(10.0 ** rs.uniform(-1.5, 0.6), np.array([1.5, -2.25, 0.75])) for _ in range(300)]
    for _ in range(150):
        c = np.round(rs.uniform(-20, 20, 3) / (2 * g)) * (2 * g)
        tris += [centred(10.0 ** rs.uniform(-1.0, 0.3), c), centred(10.0 ** rs.uniform(-1.0, 0.3), c)]
    return _soup(tris)


def flat():
    """3A. a jittered 30 x 30 grid of quads, every vertex at z = 1.5: no extent in z"""
    rs = np.random.RandomState(7200)
    m = 30
    x, y = np.meshgrid(np.linspace(-9, 9, m + 1), np.linspace(-7, 7, m + 1), indexing="ij")
    p = np.stack([x + rs.uniform(-0.1, 0.1, x.shape), y + rs.uniform(-0.1, 0.1, x.shape), np.full(x.shape, 1.5)], -1)
    tris = []
    for i in range(m):
        for j in range(m):
            tris += [[p[i, j], p[i + 1, j], p[i + 1, j + 1]], [p[i, j], p[i + 1, j + 1], p[i, j + 1]]]
    return _soup(tris)


def strip():
    """3B. 1,500 triangles of 0.1 .. 0.3 m in a 400 m x 0.5 m x 0.5 m strip"""
    rs = np.random.RandomState(7300)
    n = 1500
    cen = np.stack([rs.uniform(-200, 200, n), rs.uniform(-0.15, 0.15, n), rs.uniform(-0.15, 0.15, n)], -1)
    tri = cen[:, None, :] + rs.uniform(-0.1, 0.1, (n, 3, 3))
    tri[0, 0] = [-200.0, -0.25, -0.25]; tri[1, 0] = [200.0, 0.25, 0.25]                         # the stated extent, exactly
    return _soup(tri)


def capped(offset=None):
    """4 / 5. a 31 x 31 terrain of 0.2 m triangles (1,922 faces) crossed by two faces 80 m and 99 m long: one along x, one
    tilted and diagonal to the grid.  `offset` translates everything (in f64, before the rounding to f32).  The huge faces come
    last: scene["huge"]."""
    rs = np.random.RandomState(7400)
    m = 31
    g = np.linspace(-3.1, 3.1, m + 1)
    z = rs.normal(0.0, 0.03, (m + 1, m + 1))
    tris = []
    for i in range(m):
        for j in range(m):
            p = [[g[i], g[j], z[i, j]], [g[i + 1], g[j], z[i + 1, j]], [g[i + 1], g[j + 1], z[i + 1, j + 1]], [g[i], g[j + 1], z[i, j + 1]]]
            tris += [[p[0], p[1], p[2]], [p[0], p[2], p[3]]]
    tris.append([[-40.0, 1.0, 0.5], [40.0, 1.0, 0.5], [40.0, 1.7, 0.9]])
    tris.append([[-35.0, -35.3, -0.6], [35.0, 34.7, 1.4], [34.4, 35.5, 1.9]])
    t = np.asarray(tris, np.float64)
    if offset is not None:
        t = t + np.asarray(offset, np.float64)
    v, f = _soup(t)
    return v, f, np.array([len(f) - 2, len(f) - 1])


def chain():
    """6. three triangles of 5 cm at each x = 100 m * 2^-k, k = 0 .. 20, 0.3 m apart in y: the radix tree over their Morton
    codes peels one position after the other"""
    rs = np.random.RandomState(7500)
    k = np.repeat(np.arange(21), 3)
    cen = np.stack([100.0 * 2.0 ** -k, np.tile([0.0, 0.3, 0.6], 21), np.zeros(63)], -1)
    tri = np.einsum("nij,kj->nki", _rotations(rs, 63), _UNIT * 0.06) + cen[:, None, :]
    return _soup(tri)


N_DEGENERATE = 16


def degenerate():
    """7. separated(257), then 16 faces without area: collinear corners (eight; four of them 20 .. 40 m long and oblique, so
    their boxes span the scene) and two identical corners (eight, four of them long)"""
    v, f = separated(257)
    rs = np.random.RandomState(7600)
    extra = []
    for i in range(N_DEGENERATE):
        a = np.round(rs.uniform(2.0, 22.0, 3) * 64.0) / 64.0                                   # multiples of 2^-6 and 2^-5: the corners
        u = rs.normal(0, 1, 3); u /= np.linalg.norm(u)                                         # below are exact in f32, the area is 0
        u = np.round(u * (rs.uniform(20.0, 40.0) if i % 4 < 2 else rs.uniform(0.3, 1.0)) * 32.0) / 32.0
        a = a - 0.5 * u
        extra.append([a, a + 0.5 * u, a + u] if i < 8 else [a, a, a + u])
    e = np.asarray(extra, np.float64)
    v2 = np.concatenate([v, e.reshape(-1, 3).astype(np.float32)])
    return v2, np.arange(len(v2), dtype=np.uint32).reshape(-1, 3)


# ---- rays -------------------------------------------------------------------------------------------------------------
def _aim(rs, p, nrm, hmin=0.05, hmax=0.5, tilt=0.2):
    """rays at the points p of faces with unit normals nrm, from hmin .. hmax off the face on either side, tilted by up to `tilt`"""
    n = len(p)
    h = rs.uniform(hmin, hmax, (n, 1)) * rs.choice([-1.0, 1.0], (n, 1))
    lat = rs.normal(0, 1, (n, 3)); lat -= (lat * nrm).sum(1, keepdims=True) * nrm
    lat /= np.linalg.norm(lat, axis=1, keepdims=True)
    o = (p + h * nrm + np.abs(h) * np.tan(rs.uniform(0.0, tilt, (n, 1))) * lat).astype(np.float32)
    d = p - o
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _normals(tri):
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def _random_rays(rs, v, n, pad=2.0):
    lo, hi = v.min(0).astype(np.float64) - pad, v.max(0).astype(np.float64) + pad
    o = rs.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rs.normal(0, 1, (n, 3))
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def lattice_cells(v):
    """the cell sizes L = ext * 2 / 2^k, k = 4 .. 16, of grids that start at the scene's lower corner: where k_split's bisection
    looks for its cell size (it starts from ext * 2 and ends within the 2^16 below it)"""
    ext = float((v.max(0) - v.min(0)).max())
    return [ext * 2.0 / 2.0 ** k for k in LATTICE_K]


def lattice_points(rs, v, tri, per_k):
    """points of the face `tri` [3][3] within 1e-4 m of a grid plane org + j L (L of lattice_cells, a random axis in which the
    face is long, a random j): [len(LATTICE_K) * per_k][3]"""
    org = v.min(0).astype(np.float64)
    lo, hi = tri.min(0), tri.max(0)
    long_axes = np.flatnonzero(hi - lo > 0.5 * (hi - lo).max())
    edges = np.roll(tri, -1, 0) - tri
    e = edges[np.argmax(np.linalg.norm(edges, axis=1))]                                          # the longest edge
    e /= np.linalg.norm(e)
    out = []
    for L in lattice_cells(v):
        got = 0
        while got < per_k:
            ax = int(rs.choice(long_axes))
            r1, r2 = np.sqrt(rs.uniform()), rs.uniform()
            p = (1 - r1) * tri[0] + r1 * (1 - r2) * tri[1] + r1 * r2 * tri[2]
            j = np.round((p[ax] - org[ax]) / L)
            p = p + e * ((org[ax] + j * L + rs.uniform(-1e-4, 1e-4) - p[ax]) / e[ax])          # slide along the longest edge
            b = np.linalg.lstsq(np.stack([tri[1] - tri[0], tri[2] - tri[0]], 1), p - tri[0], rcond=None)[0]
            if b[0] > 0.002 and b[1] > 0.002 and b[0] + b[1] < 0.998:
                out.append(p); got += 1
    return np.array(out)


def _rays_of(name, v, f, huge):
    kind = name.split(":")[0]
    rs = np.random.RandomState(8000 + sum(map(ord, kind if kind == "capped" else name)))      # (the far copy: the same rays, moved)
    tri = v[f].astype(np.float64)
    o, d, aim = [], [], []

    def add(oo, dd, a=None):
        o.append(oo); d.append(dd); aim.append(np.full(len(oo), -1, np.int64) if a is None else np.asarray(a, np.int64))

    def aimed(faces, per_face, **kw):
        k = np.repeat(np.asarray(faces), per_face)
        r1, r2 = np.sqrt(rs.uniform(0, 1, (len(k), 1))), rs.uniform(0, 1, (len(k), 1))
        p = (1 - r1) * tri[k, 0] + r1 * (1 - r2) * tri[k, 1] + r1 * r2 * tri[k, 2]
        add(*_aim(rs, p, _normals(tri[k]), **kw), a=k)

    if kind in ("separated", "degenerate"):
        n = 257 if kind == "degenerate" else len(f)
        aimed(np.arange(n), max(2, 1500 // n))
        add(*_random_rays(rs, v[:3 * n], 1000))
        if kind == "degenerate":
            # across the faces without area and along them, 1 .. 20 mm beside their segment: inside their boxes, where a tree
            # must look at them.  Not AT the segment: the f32 triangle test of oracle and kernel alike has rounding noise for
            # the determinant of a face of exactly no area, the grazing guard's bound is 0 for it, and 3 of 400 rays aimed at
            # points of the segments came back as hits on such a face from the brute-force loop itself
            seg = tri[n:]
            a, b = seg[:, 0], seg[:, 2]
            u = rs.uniform(0, 1, (400, 1)); k = rs.randint(0, len(seg), 400)
            dirn = rs.normal(0, 1, (400, 3)); dirn /= np.linalg.norm(dirn, axis=1, keepdims=True)
            along = (b - a) / np.linalg.norm(b - a, axis=1, keepdims=True)
            side = np.cross(dirn, along[k]); side /= np.linalg.norm(side, axis=1, keepdims=True)
            p = a[k] + u * (b[k] - a[k]) + side * rs.uniform(1e-3, 2e-2, (400, 1)) * rs.choice([-1.0, 1.0], (400, 1))
            add((p - dirn * rs.uniform(0.5, 3.0, (400, 1))).astype(np.float32), dirn.astype(np.float32))
            off = np.cross(along, [0.3, 0.5, 0.8]); off *= 2e-3 / np.linalg.norm(off, axis=1, keepdims=True)
            add((a - 1.0 * along + off).astype(np.float32), along.astype(np.float32))
            add((b + 1.0 * along + off).astype(np.float32), (-along).astype(np.float32))
    elif kind == "coincident":
        c = 0.5 * (tri[0].min(0) + tri[0].max(0))
        dirn = rs.normal(0, 1, (600, 3)); dirn /= np.linalg.norm(dirn, axis=1, keepdims=True)
        through = c + np.where(rs.uniform(0, 1, (600, 1)) < 0.5, 0.0, rs.normal(0, 0.02, (600, 3)))
        add((through - dirn * rs.uniform(5.0, 25.0, (600, 1))).astype(np.float32), dirn.astype(np.float32))
        area = np.linalg.norm(np.cross(tri[:300, 1] - tri[:300, 0], tri[:300, 2] - tri[:300, 0]), axis=1)
        aimed(np.argsort(area)[-60:], 15, hmin=0.5, hmax=6.0)                                    # the rings only large ones cover
        aimed(300 + rs.permutation(300)[:200], 3, hmin=0.05, hmax=2.0)
        add(*_random_rays(rs, v, 700))
    elif kind in ("flat", "strip"):
        aimed(rs.permutation(len(f))[:500], 2, tilt=0.05)                                        # head-on
        n = 1200
        k = rs.randint(0, len(f), n)
        p = tri[k].mean(1)
        el = rs.uniform(0.03, 0.2, (n, 1)) * rs.choice([-1.0, 1.0], (n, 1))                      # 1.7 .. 11 degrees off the plane
        az = rs.uniform(0, 2 * np.pi, (n, 1)) if kind == "flat" else rs.choice([0.0, np.pi], (n, 1)) + rs.normal(0, 0.002, (n, 1))
        dirn = np.concatenate([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], 1)
        add((p - dirn * rs.uniform(0.5, 60.0, (n, 1))).astype(np.float32), dirn.astype(np.float32))
        add(*_random_rays(rs, v, 500, pad=1.0))
    elif kind == "capped":
        for h in huge:
            aimed([h], AIMED_PER_HUGE)
            p = lattice_points(rs, v, tri[h], LATTICE_PER_K)
            add(*_aim(rs, p, np.repeat(_normals(tri[h:h + 1]), len(p), 0)), a=np.full(len(p), h))
        aimed(rs.permutation(len(f) - 2)[:600], 1)
        add(*_random_rays(rs, v[:-6], 700))
        add(*_random_rays(rs, v, 500))
    elif kind == "chain":
        aimed(np.arange(len(f)), 30, hmin=0.02, hmax=0.3)
        p = tri[rs.randint(0, len(f), 300)].mean(1)
        add((p + [[-1.0, 0.0, 0.0]] + rs.normal(0, 0.01, (300, 3))).astype(np.float32), np.tile(np.float32([[1, 0, 0]]), (300, 1)))
        add(*_random_rays(rs, v, 300, pad=0.5))
    else:
        raise KeyError(name)
    return (np.ascontiguousarray(np.concatenate(o), np.float32), np.ascontiguousarray(np.concatenate(d), np.float32),
            np.concatenate(aim))


# ---- the grazing guard's residual class -------------------------------------------------------------------------------
def residual_class(v, f, o, d, t, face):
    """per ray: its brute-force hit is one the grazing guard looks at (det^2 < 2.5e-5 |e1 x e2|^2, here with four times that
    bound) AND lies outside the exact triangle (f64 barycentrics): a hit a tree finds only if the ray happens to cross the box
    the face -- or a clipped part of it -- is filed under.  A hit inside the exact triangle lies inside a
    part's box, whatever the incidence."""
    hit = np.flatnonzero(t >= 0)
    tri = v[f[face[hit].astype(np.int64)]].astype(np.float64)
    O, D = o[hit].astype(np.float64), d[hit].astype(np.float64)
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    pv = np.cross(D, e2)
    det = (e1 * pv).sum(1)
    nn = (np.cross(e1, e2) ** 2).sum(1)
    tv = O - tri[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (tv * pv).sum(1) / det
        w = (D * np.cross(tv, e1)).sum(1) / det
    outside = ~((u >= 0) & (w >= 0) & (u + w <= 1))
    out = np.zeros(len(t), bool)
    out[hit] = (det * det < 1e-4 * nn) & outside
    return out


# ---- cases: scene + rays + brute force, once --------------------------------------------------------------------------
CASES = tuple("separated:%d" % n for n in COUNTS) + ("coincident", "flat", "strip", "capped", "capped:far", "chain", "degenerate")
_CACHE = {}


def scene(name):
    """(verts, faces, huge face ids)"""
    kind, _, arg = name.partition(":")
    if kind == "separated":
        return separated(int(arg)) + (np.zeros(0, np.int64),)
    if kind == "capped":
        return capped(FAR_OFFSET if arg == "far" else None)
    v, f = {"coincident": coincident, "flat": flat, "strip": strip, "chain": chain, "degenerate": degenerate}[kind]()
    return v, f, np.zeros(0, np.int64)


def case(oracle, name):
    """one case: its mesh, its rays and the brute-force answer for them (read-only).  The keys are those
    assert_trace_equals_brute_force (tests/common.py) reads."""
    if name not in _CACHE:
        v, f, huge = scene(name)
        o, d, aim = _rays_of(name, v, f, huge)
        t, face = R.brute_force(oracle, v, f, o, d)
        st = {"name": name, "verts": v, "faces": f, "huge": huge, "o": o, "d": d, "aim": aim, "t": t, "face": face}
        for a in st.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[name] = st
    return _CACHE[name]


# ---- rr_lbvh.hip restated: clip_tri_box, k_split, the bisection, k_prim ------------------------------------------------
def clip_tri_box(a, b, c, clo, chi):
    """clip_tri_box for the cells [clo[i], chi[i]] of one triangle at once, operation by operation in f32: (non-empty [C],
    box lo [C][3], box hi [C][3])"""
    C = len(clo)
    rows = np.arange(C)
    p = np.zeros((C, 10, 3), f32)
    p[:, 0], p[:, 1], p[:, 2] = a, b, c
    n = np.full(C, 3)
    for axis in range(3):
        for side in range(2):
            plane = (clo if side == 0 else chi)[:, axis]
            q = np.zeros_like(p)
            m = np.zeros(C, np.int64)
            for i in range(int(n.max()) if C else 0):
                act = i < n
                u, w = p[:, i], p[rows, (i + 1) % np.maximum(n, 1)]
                inu = u[:, axis] >= plane if side == 0 else u[:, axis] <= plane
                inw = w[:, axis] >= plane if side == 0 else w[:, axis] <= plane
                keep = act & inu
                q[rows[keep], m[keep]] = u[keep]
                m[keep] += 1
                cut = act & (inu != inw)
                with np.errstate(divide="ignore", invalid="ignore"):
                    t = ((plane - u[:, axis]) / (w[:, axis] - u[:, axis])).astype(f32)
                    x = (u + (t[:, None] * (w - u).astype(f32)).astype(f32)).astype(f32)
                x[:, axis] = plane
                q[rows[cut], m[cut]] = x[cut]
                m[cut] += 1
            n, p = m, q
    ok = n > 0
    valid = np.arange(10)[None, :, None] < n[:, None, None]
    lo = np.where(valid, p, f32(3.0e38)).min(1)
    hi = np.where(valid, p, f32(-3.0e38)).max(1)
    with np.errstate(over="ignore"):                                        # (the empty cells' sentinels)
        e = (f32(1e-6) * (np.abs(lo) + np.abs(hi)).astype(f32)).astype(f32) + f32(1e-30)
        lo = np.maximum((lo - e).astype(f32), (clo - e).astype(f32))
        hi = np.minimum((hi + e).astype(f32), (chi + e).astype(f32))
    return ok, lo, hi


def cut_threshold(v, f):
    """k_side and its host end: faces whose longest box side is at most this (twice the mean longest side, summed in 32-bit
    fixed point of the extent) are never cut"""
    tri = v[f]
    ext = f32((v.max(0) - v.min(0)).max())
    if not ext > 0:
        return f32(0.0)
    s1 = f32(1.0) / ext
    side = (tri.max(1) - tri.min(1)).astype(f32).max(1)
    q = np.minimum((side * s1).astype(f32) * f32(4294967296.0), f32(4294967296.0)).astype(np.uint64)
    return f32(2.0 * (float(q.sum(dtype=np.uint64)) / len(f) / 4294967296.0) * float(ext))


def split_face(a, b, c, L, org, min_side=0.0):
    """k_split for one face: its references' boxes ([n][3] lo, [n][3] hi) and, for a report, their cells ([n][3] indices, -1
    for a face kept whole)"""
    a, b, c, org, L = f32(a), f32(b), f32(c), f32(org), f32(L)
    blo, bhi = np.minimum(a, np.minimum(b, c)), np.maximum(a, np.maximum(b, c))
    ext = (bhi - blo).astype(f32)
    cell = np.where(ext > f32(L * f32(K_MAX_CELLS)), (ext / f32(K_MAX_CELLS)).astype(f32), L).astype(f32)
    i0 = np.floor(((blo - org).astype(f32) / cell).astype(f32)).astype(np.int64)
    nc = np.floor(((bhi - org).astype(f32) / cell).astype(f32)).astype(np.int64) - i0 + 1
    nc = np.maximum(1, np.minimum(nc, K_MAX_CELLS + 1))
    whole = (blo[None], bhi[None], np.full((1, 3), -1))
    if nc.prod() == 1 or not ext.max() > f32(min_side):
        return whole
    idx = np.stack(np.meshgrid(np.arange(nc[0]), np.arange(nc[1]), np.arange(nc[2]), indexing="ij"), -1).reshape(-1, 3)
    idx = idx[np.lexsort((idx[:, 0], idx[:, 1], idx[:, 2]))]                                       # x fastest, as the kernel's loops
    at = lambda j: (org + ((i0 + j).astype(f32) * cell).astype(f32)).astype(f32)
    clo = np.where(idx == 0, blo, at(idx)).astype(f32)
    chi = np.where(idx == nc - 1, bhi, at(idx + 1)).astype(f32)
    ok, lo, hi = clip_tri_box(a, b, c, clo, chi)
    if not ok.any():
        return whole
    return lo[ok], hi[ok], idx[ok]


def split_mesh(v, f, L):
    """k_split<true> over a mesh: (box lo [n_refs][3], box hi, face of each reference)"""
    org = v.min(0)
    min_side = cut_threshold(v, f)
    lo, hi, face = [], [], []
    for i, (a, b, c) in enumerate(v[f]):
        l, h, _ = split_face(a, b, c, L, org, min_side)
        lo.append(l); hi.append(h); face.append(np.full(len(l), i))
    return np.concatenate(lo), np.concatenate(hi), np.concatenate(face)


def settle_cell(v, f, no_split=False):
    """the bisection of build_bvh4_gpu: (L, n_refs, ref_limit)"""
    nf = len(f)
    ext = f32((v.max(0) - v.min(0)).max())
    limit = nf + nf // 4 + 64
    L = f32(max(ext, f32(1e-20)) * f32(2.0))
    count = lambda cell: len(split_mesh(v, f, cell)[2])
    if not no_split and ext > 0:
        lo_l, hi_l = f32(L / f32(65536.0)), L
        for _ in range(14):
            mid = f32(np.sqrt(f32(lo_l * hi_l)))
            if count(mid) <= limit:
                hi_l = mid
            else:
                lo_l = mid
        L = hi_l
    return L, count(L), limit


def morton_keys(v, lo, hi):
    """k_prim: the 63-bit code of each reference box's centre"""
    slo = v.min(0)
    ext = f32((v.max(0) - slo).max())
    s1 = f32(1.0) / ext if ext > 0 else f32(0.0)
    cen = (((f32(0.5) * (lo + hi).astype(f32)).astype(f32) - slo).astype(f32) * s1).astype(f32)
    q = np.minimum(np.maximum((cen * f32(2097152.0)).astype(f32), f32(0.0)), f32(2097151.0)).astype(np.uint64)
    key = np.zeros(len(q), np.uint64)
    for bit in range(21):
        for k in range(3):
            key |= ((q[:, k] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + k)
    return key


def sample_face(rs, tri, n):
    """n points of the face in f64 barycentrics, rounded to f32"""
    r1, r2 = np.sqrt(rs.uniform(0, 1, (n, 1))), rs.uniform(0, 1, (n, 1))
    t = np.asarray(tri, np.float32).astype(np.float64)
    return ((1 - r1) * t[0] + r1 * (1 - r2) * t[1] + r1 * r2 * t[2]).astype(np.float32)
