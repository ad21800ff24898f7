"""numpy restatement of the windowed CFAR detectors (include/radarays_mi355.h, rr_window.hip), straight from the definition.

`cell` is the definition word for word: loops over the window, a list of training values, `sorted`, the r-th.  `masks` applies the
same definition to a whole image at once -- one shifted copy of the image per window offset, summed or sorted along the offsets --
and tests/test_window_host.py holds it to `cell`.  Neither borrows from the kernel's route: no row sums, no sliding sums, no
threshold table.  float32 where the header says f32, one rounding per operation."""
import numpy as np

from radarays_ros_amd.native import POINT_DTYPE

DEFAULTS = dict(method=3, guard_range=2, train_range=16, guard_azimuth=1, train_azimuth=2, rank_permille=750, min_intensity=1, min_bin=0,
                scale=3.0)
CA, GO, SO, OS = 0, 1, 2, 3


def config(**kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(DEFAULTS, **kw)


def _ca(z, n, S, scale):
    return bool(np.float32(z * n) > np.float32(scale) * np.float32(S))


def cell(img, i, c, cfg):
    """is (bin i, column c) of one image [n_cells][n_angles] a detection"""
    cfg = config(**cfg)
    N, A = img.shape
    Gr, Ga = cfg["guard_range"], cfg["guard_azimuth"]
    Hr, Hc = Gr + cfg["train_range"], Ga + cfg["train_azimuth"]
    z = int(img[i, c])
    near, far, row = [], [], []
    for db in range(-Hr, Hr + 1):
        b = i + db
        if b < 0 or b >= N:
            continue
        for dc in range(-Hc, Hc + 1):
            if abs(db) <= Gr and abs(dc) <= Ga:
                continue
            (near if db < 0 else far if db > 0 else row).append(int(img[b, (c + dc) % A]))
    train = near + row + far
    n = len(train)
    if i < cfg["min_bin"] or z < cfg["min_intensity"] or n == 0:
        return False
    m = cfg["method"]
    if m == CA:
        return _ca(z, n, sum(train), cfg["scale"])
    if m == OS:
        r = max(1, (n * cfg["rank_permille"] + 999) // 1000)
        v = sorted(train)[r - 1]
        return bool(np.float32(z) > np.float32(cfg["scale"]) * np.float32(v))
    if not near and not far:
        return False
    if not near:
        half = far
    elif not far:
        half = near
    else:
        a, b = sum(near) * len(far), sum(far) * len(near)           # mean(near) against mean(far), exactly
        half = near if (a >= b if m == GO else a <= b) else far
    return _ca(z, len(half), sum(half), cfg["scale"])


def masks(img, cfg):
    """{method: bool [n_cells][n_angles]} for all four methods of one image under one window (cfg's method is ignored)"""
    cfg = config(**cfg)
    z = np.asarray(img).astype(np.int64)
    N, A = z.shape
    Gr, Ga = cfg["guard_range"], cfg["guard_azimuth"]
    Hr, Hc = Gr + cfg["train_range"], Ga + cfg["train_azimuth"]
    assert 2 * Hc + 1 <= A
    rows = np.arange(N)
    vals, valid, side = [], [], []
    for db in range(-Hr, Hr + 1):
        ok = (rows + db >= 0) & (rows + db < N)
        src = np.clip(rows + db, 0, N - 1)
        for dc in range(-Hc, Hc + 1):
            if abs(db) <= Gr and abs(dc) <= Ga:
                continue
            vals.append(np.roll(z[src], -dc, axis=1).astype(np.int16))     # [i][c] = z[i + db][(c + dc) mod A]
            valid.append(np.broadcast_to(ok[:, None], z.shape))
            side.append(-1 if db < 0 else 1 if db > 0 else 0)
    vals, valid, side = np.stack(vals), np.stack(valid), np.asarray(side)[:, None, None]
    f32 = np.float32
    scale = f32(cfg["scale"])

    def ca(n, S):
        return (n > 0) & ((z * n).astype(f32) > scale * S.astype(f32))

    def count_sum(sel):
        w = valid & sel
        return w.sum(axis=0, dtype=np.int64), np.where(w, vals, 0).sum(axis=0, dtype=np.int64)

    n, S = count_sum(np.ones_like(side, bool))
    nn, Sn = count_sum(side < 0)
    nf, Sf = count_sum(side > 0)
    cand = (z >= cfg["min_intensity"]) & (rows[:, None] >= cfg["min_bin"]) & (n > 0)
    out = {CA: cand & ca(n, S)}
    a, b = Sn * nf, Sf * nn
    for m, near_wins in ((GO, a >= b), (SO, a <= b)):
        near = np.where(nn == 0, False, np.where(nf == 0, True, near_wins))
        out[m] = cand & np.where(near, ca(nn, Sn), ca(nf, Sf))
    order = np.sort(np.where(valid, vals, np.int16(256)), axis=0)      # the training values ascending, the clipped ones last
    r = np.maximum(1, (n * cfg["rank_permille"] + 999) // 1000)
    v = np.take_along_axis(order, np.clip(r - 1, 0, len(order) - 1)[None], axis=0)[0].astype(np.int64)
    out[OS] = cand & (z.astype(f32) > scale * v.astype(f32))
    return out


def points_of(img, mask, scroll=0, theta_min=0.0, theta_inc=-2 * np.pi / 400, resolution=0.0438):
    """a detection mask -> (points POINT_DTYPE sorted by column then bin, offsets uint32 [n_angles + 1]): rr_detect's output rule"""
    img = np.asarray(img)
    N, A = img.shape
    col, b = np.nonzero(mask.T)
    offs = np.zeros(A + 1, np.uint32)
    offs[1:] = np.cumsum(mask.sum(axis=0))
    a = (col - int(scroll)) % A
    theta = np.float32(theta_min) + a.astype(np.float32) * np.float32(theta_inc)
    r = ((b.astype(np.float64) + 0.5) * float(resolution)).astype(np.float32)
    pts = np.zeros(len(col), POINT_DTYPE)
    pts["x"] = r * np.cos(theta)
    pts["y"] = r * np.sin(theta)
    pts["intensity"] = img[b, col].astype(np.float32)
    pts["column"] = col
    pts["bin"] = b
    return pts, offs


def wall_scene():
    """the scene of the issue: seed 3 noise below 30 at 200 bins by 37 columns, a wall of 200 in rows 90..101 -> (image, wall mask)"""
    img = np.random.RandomState(3).randint(0, 30, (200, 37)).astype(np.uint8)
    img[90:102, :] = 200
    wall = np.zeros(img.shape, bool)
    wall[90:102, :] = True
    return img, wall
