"""Oriented surface points and the point-to-line scan matcher of include/radarays_mi355.h (rr_surface_points, rr_register_surfels) restated
in numpy: f32 where the definition says f32 (numpy rounds every operation and fuses none), Python floats (IEEE f64, correctly rounded
+ - * / sqrt) for the eigen step and the solve, Python ints for every sum: whole numbers of any size, beside which the kernel's two-limb
sums are restated and held to them.  The GPU tests compare against it byte for byte; the host tests hold it to hand-worked cases."""
import math

import numpy as np

import icp_ref
from radarays_ros_amd import native

NONE = native.ICP_NONE
DEGENERATE, TRUNCATED = native.ICP_DEGENERATE, native.ICP_TRUNCATED
SF_TRUNCATED, SF_CAPPED = native.SURFELS_TRUNCATED, native.SURFELS_CAPPED
SF_RANGE = np.float32(8192.0)
LINE_RANGE = np.float32(2048.0)
xy_of, points_of, normalise = icp_ref.xy_of, icp_ref.points_of, icp_ref.normalise

# ---- the closed loop: DESIGN.md §22's own scene (icp_ref.LOOP_*: the room, the two poses, 64 azimuths, the 2 strongest returns), B's cloud
# registered onto the surface points of A's cloud.  The cell is the spacing of the points along a wall, about 1 m, chosen before any
# result was seen; 64 azimuths suffice, the 400-azimuth variant is not needed.  What the restatement gives on the oracle's images
# (test_surfels_host.py measures and prints it), beside point-to-point's 0.456 degrees and 0.1817 m on the same clouds:
LOOP_SURFELS = dict(cell=1.0, width=32, min_points=3, max_ratio=0.1)
LOOP_YAW_MEASURED, LOOP_T_MEASURED = math.radians(0.1185), 0.0654


# ---- surface points ------------------------------------------------------------------------------------------------------------------
def cell_sums(cloud, cell_q, width):
    """the six sums per occupied cell of one cloud: {linear cell: [N, Sx, Sy, Sxx, Sxy, Syy]} in Python ints"""
    x, y = xy_of(cloud)
    half = (width * cell_q) // 2
    s256 = np.float32(256.0)
    sums = {}
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (np.abs(x) < SF_RANGE) & (np.abs(y) < SF_RANGE)          # False for NaN and infinities
        X, Y = np.rint(x[ok] * s256).astype(np.int64), np.rint(y[ok] * s256).astype(np.int64)
    for U, V in zip((X + half).tolist(), (Y + half).tolist()):
        ix, iy = U // cell_q, V // cell_q                             # Python's // is the floor
        if not (0 <= ix < width and 0 <= iy < width):
            continue
        rx, ry = U - ix * cell_q, V - iy * cell_q
        s = sums.setdefault(iy * width + ix, [0] * 6)
        for k, v in enumerate((1, rx, ry, rx * rx, rx * ry, ry * ry)):
            s[k] += v
    return sums


def surfel_of(sums, cell, cell_q, width, min_points, max_ratio):
    """the record of one occupied cell as a tuple in SURFEL_DTYPE's order, or None if the keep rule drops it"""
    half = (width * cell_q) // 2
    ix, iy = cell % width, cell // width
    N = Sx = Sy = Sxx = Sxy = Syy = 0
    for b in (-1, 0, 1):
        for a in (-1, 0, 1):
            jx, jy = ix + a, iy + b
            s = sums.get(jy * width + jx) if 0 <= jx < width and 0 <= jy < width else None
            if s is None:
                continue
            n, sx, sy, sxx, sxy, syy = s
            ox, oy = a * cell_q, b * cell_q
            N += n
            Sx += sx + n * ox
            Sy += sy + n * oy
            Sxx += sxx + 2 * ox * sx + n * ox * ox
            Sxy += sxy + ox * sy + oy * sx + n * ox * oy
            Syy += syy + 2 * oy * sy + n * oy * oy
    Cxx, Cxy, Cyy = N * Sxx - Sx * Sx, N * Sxy - Sx * Sy, N * Syy - Sy * Sy
    assert max(abs(Cxx), abs(Cxy), abs(Cyy)) < 1 << 59              # the header's proof
    T, d, o = float(Cxx + Cyy), float(Cxx - Cyy), float(2 * Cxy)
    h = math.sqrt(d * d + o * o)
    lmax, v = (T + h) / 2.0, (T - h) / 2.0
    lmin = v if v > 0.0 else 0.0
    if not (N >= min_points and h > 0.0 and lmin <= float(np.float32(max_ratio)) * lmax):
        return None
    tx, ty = (h + d, o) if d >= 0.0 else (o, h - d)
    tn = math.sqrt(tx * tx + ty * ty)
    tx, ty = tx / tn, ty / tn
    mx = float(ix * cell_q - half) + float(Sx) / float(N)
    my = float(iy * cell_q - half) + float(Sy) / float(N)
    nx, ny = -ty, tx
    if nx * mx + ny * my > 0.0:
        nx, ny = -nx, -ny
    den = (float(N) * float(N)) * 65536.0
    return (np.float32(mx / 256.0), np.float32(my / 256.0), np.float32(nx), np.float32(ny), np.float32(lmin / den), np.float32(lmax / den), N, cell)


def surface_points(clouds, cell, width, min_points=3, max_ratio=0.1, max_surfels=4096, max_points=None):
    """n clouds -> (a list of n SURFEL_DTYPE arrays: the first min(kept, max_surfels) records in ascending cell order, counts uint32 [n][2])"""
    cell_q = native.surfel_cell_q(cell)
    out, counts = [], np.zeros((len(clouds), 2), np.uint32)
    for f, cloud in enumerate(clouds):
        flags = 0
        if max_points is not None and len(cloud) > max_points:
            cloud, flags = cloud[:max_points], SF_TRUNCATED
        sums = cell_sums(cloud, cell_q, width)
        recs = [r for r in (surfel_of(sums, c, cell_q, width, min_points, max_ratio) for c in sorted(sums)) if r is not None]
        if len(recs) > max_surfels:
            flags |= SF_CAPPED
        counts[f] = (len(recs), flags)
        out.append(np.array(recs[:max_surfels], native.SURFEL_DTYPE) if recs[:max_surfels] else np.zeros(0, native.SURFEL_DTYPE))
    return out, counts


def surfels_of(xy, normals, var=(0.0, 1.0)):
    """[m][2] means and [m][2] normals -> SURFEL_DTYPE with variances, count and cell the matcher must ignore"""
    xy, nn = np.asarray(xy, np.float32).reshape(-1, 2), np.asarray(normals, np.float32).reshape(-1, 2)
    s = np.zeros(len(xy), native.SURFEL_DTYPE)
    s["x"], s["y"], s["nx"], s["ny"] = xy[:, 0], xy[:, 1], nn[:, 0], nn[:, 1]
    s["var_n"], s["var_t"], s["count"], s["cell"] = var[0], var[1], 77, 0xFFFFFFF0
    return s


def corridor(angle, m=40, offset=(0.1, -0.15)):
    """a corridor wall 2 m from the origin whose normal points along `angle`: (m surfels with that one normal, a source cloud `offset` away)"""
    n = (math.cos(angle), math.sin(angle))
    t = np.linspace(-5, 5, m).astype(np.float32)
    xy = np.stack([2 * n[0] - t * n[1], 2 * n[1] + t * n[0]], -1)
    return surfels_of(xy, np.tile(np.float32(n), (m, 1))), (xy + np.float32(offset)).astype(np.float32)


GENERAL_CORRIDORS = (0.3, 0.6435, 1.0, 2.2)      # radians: neither an axis nor a diagonal


# ---- point-to-line registration --------------------------------------------------------------------------------------------------------
def line_pass(sx, sy, tgt, state, gate2, chunk=256):
    """one pass: (j* uint32 [m] with NONE for an unmatched point, (N, H [3][3], g [3], rr, two) in Python ints; two: the (lo, hi) limb sums
    of a0*a0, a0*r and r*r, every term split as the kernel splits it before any reduction: t & 0xFFFFFFFF and t >> 32.  The f64 value
    (double)hi * 2^32 + (double)lo the solve sees depends on that split, so it is restated and not only the whole number)"""
    tx, ty, nx, ny = (np.ascontiguousarray(tgt[k]) for k in ("x", "y", "nx", "ny"))
    cf, sf, txf, tyf = (np.float32(v) for v in state)
    inf = np.float32(np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        px = (cf * sx - sf * sy) + txf
        py = (sf * sx + cf * sy) + tyf
        ok_t = (np.abs(tx) < LINE_RANGE) & (np.abs(ty) < LINE_RANGE) & (np.abs(nx) <= 1) & (np.abs(ny) <= 1)      # False for NaN
        qx, qy = np.where(ok_t, tx, inf), np.where(ok_t, ty, inf)
        m = len(sx)
        best = np.full(m, inf, np.float32)
        j = np.full(m, NONE, np.uint32)
        if len(tx):
            for a in range(0, m, chunk):
                dx = px[a:a + chunk, None] - qx[None, :]
                dy = py[a:a + chunk, None] - qy[None, :]
                d2 = dx * dx + dy * dy
                d2 = np.where(np.isnan(d2), inf, d2)                 # a NaN never wins
                k = np.argmin(d2, axis=1)                            # the first of equal minima: the lower index
                b = d2[np.arange(len(k)), k]
                won = b < inf
                best[a:a + chunk] = np.where(won, b, inf)
                j[a:a + chunk] = np.where(won, k, NONE).astype(np.uint32)
        matched = (np.abs(px) < LINE_RANGE) & (np.abs(py) < LINE_RANGE) & (j != NONE) & (best <= gate2)
        j = np.where(matched, j, NONE).astype(np.uint32)
        jm = j[matched].astype(np.int64)
        s64, s1024 = np.float32(64.0), np.float32(1024.0)
        Px, Py = np.rint(px[matched] * s64).astype(np.int64).tolist(), np.rint(py[matched] * s64).astype(np.int64).tolist()
        Qx, Qy = np.rint(tx[jm] * s64).astype(np.int64).tolist(), np.rint(ty[jm] * s64).astype(np.int64).tolist()
        Mx, My = np.rint(nx[jm] * s1024).astype(np.int64).tolist(), np.rint(ny[jm] * s1024).astype(np.int64).tolist()
    N, H, g, rr, two = 0, [[0] * 3 for _ in range(3)], [0] * 3, 0, [[0, 0], [0, 0], [0, 0]]
    for k in range(len(Px)):                                          # Python ints: whole numbers of any size
        r = Mx[k] * (Px[k] - Qx[k]) + My[k] * (Py[k] - Qy[k])
        a = (Px[k] * My[k] - Py[k] * Mx[k], Mx[k], My[k])
        assert abs(r) <= 1 << 29 and abs(a[0]) <= 1 << 28            # the header's bounds
        N += 1
        for u in range(3):
            g[u] += a[u] * r
            for v in range(3):
                H[u][v] += a[u] * a[v]
        rr += r * r
        for w, t in enumerate((a[0] * a[0], a[0] * r, r * r)):
            two[w][0] += t & 0xFFFFFFFF
            two[w][1] += t >> 32
    for w, whole in enumerate((H[0][0], g[0], rr)):
        assert two[w][1] * 4294967296 + two[w][0] == whole          # the limbs are the whole number
    return j, (N, H, g, rr, [tuple(v) for v in two])


def join(lo, hi):
    return float(hi) * 4294967296.0 + float(lo)


def solve(state, N, H, g, two_limb):
    """one solve: (the new state, degenerate?).  two_limb: ((lo, hi) of H00, (lo, hi) of g0) as the kernel's sums hold them"""
    c, s, tx, ty = state
    if N < 3:
        return state, True
    H00, g0 = join(*two_limb[0]), join(*two_limb[1])
    H01, H02, H11, H12, H22 = float(H[0][1]), float(H[0][2]), float(H[1][1]), float(H[1][2]), float(H[2][2])
    g1, g2 = float(g[1]), float(g[2])
    d0 = H00
    if not d0 > 0.0:
        return state, True
    l10, l20 = H01 / d0, H02 / d0
    d1 = H11 - l10 * H01
    if not d1 > 0.0:
        return state, True
    m21 = H12 - l20 * H01
    l21 = m21 / d1
    d2 = (H22 - l20 * H02) - l21 * m21
    if not d2 > 0.0:
        return state, True
    z0 = -g0
    z1 = -g1 - l10 * z0
    z2 = (-g2 - l20 * z0) - l21 * z1
    x2 = z2 / d2
    x1 = z1 / d1 - l21 * x2
    x0 = (z0 / d0 - l10 * x1) - l20 * x2
    u = x0 / 2.0
    dc, ds = (1.0 - u * u) / (1.0 + u * u), (2.0 * u) / (1.0 + u * u)
    dtx, dty = x1 / 64.0, x2 / 64.0
    c1 = dc * c - ds * s
    s1 = ds * c + dc * s
    tx1 = (dc * tx - ds * ty) + dtx
    ty1 = (ds * tx + dc * ty) + dty
    n = math.sqrt(c1 * c1 + s1 * s1)
    return (c1 / n, s1 / n, tx1, ty1), False


def sse_of(rr_limbs):
    lo, hi = rr_limbs
    return 0x7FFFFFFFFFFFFFFF if hi >= 1 << 30 else hi * 4294967296 + lo


def register(sources, target, init=None, gate=1.0, iterations=10, max_points=None, max_tgt=None):
    """n source clouds against one SURFEL_DTYPE target -> (records ICP_DTYPE [n], states float64 [iterations + 1][n][4]: the state each
    pass ran at, a list of n uint32 arrays: the last pass's j* per point).  A cloud longer than max_points / max_tgt is cut and flagged."""
    n = len(sources)
    tgt = np.asarray(target)
    t_trunc = max_tgt is not None and len(tgt) > max_tgt
    if t_trunc:
        tgt = tgt[:max_tgt]
    g = np.float32(gate)
    gate2 = g * g
    recs = np.zeros(n, native.ICP_DTYPE)
    states = np.zeros((iterations + 1, n, 4), np.float64)
    corr = []
    for f in range(n):
        sx, sy = xy_of(sources[f])
        flags = 0
        if max_points is not None and len(sx) > max_points:
            sx, sy, flags = sx[:max_points], sy[:max_points], TRUNCATED
        if t_trunc:
            flags |= TRUNCATED
        state = (1.0, 0.0, 0.0, 0.0)
        if init is not None:
            state, deg = normalise(init[f])
            flags |= deg
        for it in range(iterations):
            states[it, f] = state
            _, (N, H, gg, _, two) = line_pass(sx, sy, tgt, state, gate2)
            state, deg = solve(state, N, H, gg, two[:2])
            if deg:
                flags |= DEGENERATE
        states[iterations, f] = state
        j, (N, _, _, _, two) = line_pass(sx, sy, tgt, state, gate2)
        recs[f] = (state[0], state[1], state[2], state[3], sse_of(two[2]), N, flags)
        corr.append(j)
    return recs, states, corr


def errors(rec, truth):
    """(|yaw error| in radians, translation error in metres) of a record against the true transform (x, y, yaw)"""
    return icp_ref.loop_errors(rec, truth)
