"""Plain helpers of the dynamic-scene tests (tests/test_gpu_dynamic.py, tests/test_gpu_dynamic_splits.py): the posed triangle
soup in the library's f32 arithmetic, and a scene that both tree builders CUT (a fine terrain crossed by huge faces) with
moving parts where a refit has the most to decide, its states, the rays that probe them and the brute-force side.

Nothing here needs a GPU.  The reference of every state is the oracle's brute-force loop over the posed soup; it is computed
once per state and process (state()) and shared, unchanged, by every test that asks for it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz"))

IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)


# ---- the posed soup, with the library's arithmetic --------------------------------------------------------------------
def q_rot(q, v):
    """rr_device.h q_rot in its term order, float32, un-fused; q [n][4], v [n][3]"""
    q = q.astype(np.float32); v = v.astype(np.float32)
    qx, qy, qz, qw = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    vx, vy, vz = v[:, 0], v[:, 1], v[:, 2]
    tx = qw * vx + qy * vz - qz * vy
    ty = qw * vy - qx * vz + qz * vx
    tz = qw * vz + qx * vy - qy * vx
    tw = np.float32(0.0) - qx * vx - qy * vy - qz * vz
    cx, cy, cz, cw = -qx, -qy, -qz, qw
    rx = tw * cx + tx * cw + ty * cz - tz * cy
    ry = tw * cy - tx * cz + ty * cw + tz * cx
    rz = tw * cz + tx * cy - ty * cx + tz * cw
    return np.stack([rx, ry, rz], -1).astype(np.float32)


def posed_soup(scene, poses, verts=None):
    v = scene["verts"] if verts is None else verts
    f, o = scene["faces"], scene["face_object_id"]
    poses = np.asarray(poses, np.float32).reshape(-1, 7)
    corners = v[f.reshape(-1)].astype(np.float32)                # [3 nf][3]
    P = poses[np.repeat(o, 3)]
    moved = q_rot(P[:, :4], corners) + P[:, 4:]
    ident = np.all(P == IDENT, axis=1)
    moved[ident] = corners[ident]
    out = dict(scene)
    out["verts"] = moved.astype(np.float32)
    out["faces"] = np.arange(3 * len(f), dtype=np.uint32).reshape(-1, 3)
    return out


def about(center, yaw, shift=(0.0, 0.0, 0.0)):
    """a pose that turns by `yaw` about the vertical axis through `center`, then shifts"""
    q = np.array([[0, 0, np.sin(yaw / 2), np.cos(yaw / 2)]], np.float32)
    c = np.asarray(center, np.float32).reshape(1, 3)
    t = c - q_rot(q, c) + np.asarray(shift, np.float32)
    return np.concatenate([q[0], t[0]]).astype(np.float32)


def identity_poses(n):
    return np.tile(IDENT, (n, 1))


# ---- a scene that both builders split ---------------------------------------------------------------------------------
TERRAIN_CELLS = 32
N_TERRAIN_VERTS = (TERRAIN_CELLS + 1) ** 2
N_OBJECTS = 5
AIMED_PER_FACE = 250           # rays of kind (a) per huge face
N_GRAZING, N_SKIMMING, N_FUZZ, N_FUZZ_MOVING, N_RANDOM = 1200, 600, 900, 500, 400


def _box(lo, hi):
    """the 12 triangles of a closed axis-parallel box, [12][3][3]"""
    c = np.array([[lo[0], lo[1], lo[2]], [hi[0], lo[1], lo[2]], [hi[0], hi[1], lo[2]], [lo[0], hi[1], lo[2]],
                  [lo[0], lo[1], hi[2]], [hi[0], lo[1], hi[2]], [hi[0], hi[1], hi[2]], [lo[0], hi[1], hi[2]]])
    t = []
    for a, b, cc, d in ((0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 5, 4), (2, 3, 7, 6), (1, 2, 6, 5), (0, 3, 7, 4)):
        t += [[c[a], c[b], c[cc]], [c[a], c[cc], c[d]]]
    return np.array(t)


def _quad(q):
    return np.array([[q[0], q[1], q[2]], [q[0], q[2], q[3]]], np.float64)


def _wall(a, b, height, lean=(0.0, 0.0)):
    """a quad standing on the segment a-b"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    up = np.array([lean[0], lean[1], height])
    return _quad([a, b, b + up, a + up])


# the huge static faces of object 0: (a, b, height, lean); 20..40 m long
_WALLS = (((-18.0, -6.0, -0.3), (17.0, -2.0, -0.3), 2.5, (0.0, 0.0)),
          ((-5.0, -18.0, -0.2), (3.0, 18.0, 0.1), 1.2, (0.1, 0.0)),
          ((6.0, -17.0, -0.1), (16.0, 8.0, 0.0), 3.0, (0.0, 0.0)),
          ((-17.0, 12.0, 0.7), (12.0, 16.0, 0.9), 0.02, (0.04, -0.3)))      # a long sliver, almost level
_FLOOR = ((-19.0, -19.0, -1.0), (19.0, -19.0, -0.6), (19.0, 19.0, 1.0), (-19.0, 19.0, 0.6))


def _floor_z(x, y):
    u, v = (x + 19.0) / 38.0, (y + 19.0) / 38.0
    return -1.0 + 0.4 * u + 1.6 * v


def split_scene():
    """About 2,500 faces in five objects (deterministic):
      0  static: a 32 x 32 terrain over 40 m with gentle noise, crossed by a floor-sized quad, three long walls and a sliver
      1  moving: 36 small closed boxes standing on the floor quad and against the walls
      2  moving: a gate of four triangles 16 m long
      3  moving: one small box far from every large face
      4  moving: one small box that gets carried far outside
    verts / faces are indexed for the terrain (its vertices come first: update_vertices deforms them) and a plain soup for
    the rest.  scene["huge"] lists the huge faces (static ones first, then the gate's)."""
    rs = np.random.RandomState(20240)
    m = TERRAIN_CELLS
    g = np.linspace(-20.0, 20.0, m + 1)
    z = rs.normal(0.0, 0.15, (m + 1, m + 1))
    tv = np.stack([np.repeat(g, m + 1), np.tile(g, m + 1), z.reshape(-1)], -1)          # vertex i * (m + 1) + j
    tf = []
    for i in range(m):
        for j in range(m):
            a, b, c, d = i * (m + 1) + j, (i + 1) * (m + 1) + j, (i + 1) * (m + 1) + j + 1, i * (m + 1) + j + 1
            tf += [[a, b, c], [a, c, d]]
    soup, obj = [], []

    def add(tris, o):
        soup.append(np.asarray(tris, np.float64).reshape(-1, 3, 3)); obj.extend([o] * len(soup[-1]))

    add(_quad(np.array(_FLOOR)), 0)
    for a, b, h, lean in _WALLS:
        add(_wall(a, b, h, lean), 0)
    n_static_huge = 2 + 2 * len(_WALLS)
    # object 1: boxes against the three standing walls (touching the wall's plane at one edge) and on the floor quad
    for k in range(18):
        a, b, h, _ = _WALLS[k % 3]
        a = np.array(a); b = np.array(b)
        s = rs.uniform(0.2, 1.0, 3)
        along = (b - a) / np.linalg.norm(b - a)
        side = np.array([-along[1], along[0], 0.0]) * rs.choice([-1.0, 1.0])
        p = a + rs.uniform(0.05, 0.95) * (b - a)
        cen = p + side * (0.5 * (abs(side[0]) * s[0] + abs(side[1]) * s[1]))              # the nearest corner lies on the wall
        lo = np.array([cen[0] - 0.5 * s[0], cen[1] - 0.5 * s[1], p[2] + rs.uniform(0.0, 0.5 * h)])
        add(_box(lo, lo + s), 1)
    for k in range(18):
        s = rs.uniform(0.2, 1.0, 3)
        x, y = rs.uniform(-17.0, 17.0, 2)
        zs = max(_floor_z(x + dx, y + dy) for dx in (0.0, s[0]) for dy in (0.0, s[1]))      # stands on the floor quad
        lo = np.array([x, y, zs])
        add(_box(lo, lo + s), 1)
    # object 2: the gate, a standing quad and a roof
    add(_quad(np.array([[-8.0, 9.0, -0.5], [8.0, 9.0, -0.5], [8.0, 9.5, 3.5], [-8.0, 9.5, 3.5]])), 2)
    add(_quad(np.array([[-8.0, 9.5, 3.5], [8.0, 9.5, 3.5], [8.0, 13.0, 3.0], [-8.0, 13.0, 3.0]])), 2)
    add(_box(np.array([13.0, -16.0, 7.0]), np.array([13.5, -15.5, 7.5])), 3)
    add(_box(np.array([-15.5, 14.0, 2.5]), np.array([-14.9, 14.6, 3.1])), 4)
    sv = np.concatenate(soup).reshape(-1, 3)
    verts = np.concatenate([tv, sv]).astype(np.float32)
    faces = np.concatenate([np.array(tf), len(tv) + np.arange(len(sv)).reshape(-1, 3)]).astype(np.uint32)
    oid = np.concatenate([np.zeros(len(tf), np.uint32), np.array(obj, np.uint32)])
    first = len(tf)
    gate0 = first + n_static_huge + 36 * 12
    huge = np.concatenate([np.arange(first, first + n_static_huge), np.arange(gate0, gate0 + 4)])
    return {"verts": verts, "faces": faces, "face_object_id": oid, "huge": huge, "n_static_huge": n_static_huge}


def deformed_verts(scene):
    """the terrain bent (as tests/test_gpu_dynamic.py bends its heightfield); the extent stays"""
    v = scene["verts"].copy()
    n = N_TERRAIN_VERTS
    v[:n, 2] += (0.6 * np.sin(0.3 * v[:n, 0]) * np.cos(0.25 * v[:n, 1])).astype(np.float32)
    return v


def poses_of(name):
    """the pose sets of the state machine.  Everything but "far" / "copy" stays inside the extent the tree was built for."""
    P = identity_poses(N_OBJECTS)
    if name == "built":
        return P
    if name == "copy":                      # what the copied context is given: not what its source has
        P[1] = about((0.0, 0.0, 0.0), -0.03, (-0.25, 0.2, 0.05))
        P[2] = about((0.0, 11.0, 0.0), -0.4, (-1.0, -2.0, 0.2))
        P[4] = about((0.0, 0.0, 0.0), 0.0, (0.0, -140.0, 0.0))
        return P
    P[1] = about((0.0, 0.0, 0.0), 0.02, (0.3, -0.2, 0.1))
    P[3] = about((13.0, -16.0, 0.0), 0.7, (-2.0, 1.0, -1.0))
    if name in ("gate", "far"):
        P[2] = about((0.0, 11.0, 0.0), 0.6, (2.0, -3.0, 0.3))
    if name == "far":
        P[4] = about((-15.0, 14.0, 0.0), 0.3, (150.0, 0.0, 0.0))
    assert name in ("inside", "gate", "far"), name
    return P


# state name -> (pose set, deformed terrain?)
STATES = {"built": ("built", False), "inside": ("inside", False), "gate": ("gate", False), "far": ("far", False),
          "deformed": ("inside", True), "deformed_gate": ("gate", True), "deformed_far": ("far", True), "copy": ("copy", False)}


def extent_measure(v):
    """what hit_pad is 1e-5 of (rr_scene.hip guard_pad)"""
    return float(max((v.max(0) - v.min(0)).max(), np.abs(v).max()))


# ---- rays -------------------------------------------------------------------------------------------------------------
def aimed_rays(rs, v, f, huge, per_face):
    """(a) rays aimed at points spread uniformly over each huge face, from 0.05 .. 0.5 m off the face on either side, tilted
    by up to ~0.2 rad.  Returns o, d and the face each ray is aimed at."""
    tri = v[f[huge]].astype(np.float64)                                    # [h][3][3]
    n = len(huge) * per_face
    k = np.repeat(np.arange(len(huge)), per_face)
    r1, r2 = np.sqrt(rs.uniform(0, 1, (n, 1))), rs.uniform(0, 1, (n, 1))
    p = (1 - r1) * tri[k, 0] + r1 * (1 - r2) * tri[k, 1] + r1 * r2 * tri[k, 2]
    e1, e2 = tri[k, 1] - tri[k, 0], tri[k, 2] - tri[k, 0]
    nrm = np.cross(e1, e2); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    h = rs.uniform(0.05, 0.5, (n, 1)) * rs.choice([-1.0, 1.0], (n, 1))
    lat = rs.normal(0, 1, (n, 3)); lat -= (lat * nrm).sum(1, keepdims=True) * nrm
    lat /= np.linalg.norm(lat, axis=1, keepdims=True)
    o = (p + h * nrm + np.abs(h) * np.tan(rs.uniform(0.0, 0.2, (n, 1))) * lat).astype(np.float32)
    d = p - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32), huge[k]


def skimming_rays(rs, v, f, faces, pad, n):
    """(b') rays in the plane of one of `faces` that run ALONG its box, 0 .. 2.5 x pad outside it: along the side of the box
    that the face's extreme corner (or its axis-parallel edge) lies on, tilted out of the plane by 3e-7 .. 3e-4 rad.  In exact
    arithmetic such a ray misses the face; at this incidence Moeller-Trumbore in f32 accepts some of them, and the grazing
    guard keeps those whose point lies within hit_pad of the face's box.  A hierarchy finds them only if its boxes reach as
    far out as hit_pad does -- after the extent has grown, only if the as-built boxes were widened."""
    tri = v[f[faces]].astype(np.float64)
    T = tri[rs.randint(0, len(faces), n)]
    ax = rs.randint(0, 3, n); side = rs.choice([-1.0, 1.0], n)
    nrm = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    e = np.eye(3)[ax]
    along = np.cross(nrm, e); along /= np.linalg.norm(along, axis=1, keepdims=True)      # in the plane, the coordinate stays
    out = e - (e * nrm).sum(1, keepdims=True) * nrm                                      # in the plane, the coordinate grows fastest
    coord = (T * e[:, None, :]).sum(2) * side[:, None]
    order = np.argsort(coord, axis=1)
    i = np.arange(n)
    top, second = T[i, order[:, 2]], T[i, order[:, 1]]
    is_edge = np.abs(coord[i, order[:, 2]] - coord[i, order[:, 1]]) < 1e-9
    p = top + np.where(is_edge, rs.uniform(0, 1, n), 0.0)[:, None] * (second - top)
    p = p + side[:, None] * out * (rs.uniform(0.0, 2.5, (n, 1)) * pad) / (out * e).sum(1, keepdims=True)
    tilt = 10.0 ** rs.uniform(-6.5, -3.5, (n, 1)) * rs.choice([-1.0, 1.0], (n, 1))
    d = along * rs.choice([-1.0, 1.0], (n, 1)) + tilt * nrm
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = p - d * rs.uniform(1.0, 30.0, (n, 1))
    return o.astype(np.float32), d.astype(np.float32)


def misses_boxes(o, d, lo, hi):
    """per ray: the ray (t >= 0) has no point in its box [lo, hi]; the slab test in f64"""
    o = o.astype(np.float64); d = d.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (lo - o) / d, (hi - o) / d
    inside = (o >= lo) & (o <= hi)
    tn = np.where(d == 0, np.where(inside, -np.inf, np.inf), np.minimum(t1, t2))
    tf = np.where(d == 0, np.where(inside, np.inf, -np.inf), np.maximum(t1, t2))
    return ~(np.maximum(tn.max(1), 0.0) <= tf.min(1))


def probe_rays(seed, v, f, huge, moving, static_huge):
    """the ~7,000 rays of one state: (a) aimed at the huge faces, (b) grazing the largest faces next to their edges and
    skimming the boxes of the static huge faces just outside them,
    (c) the nasty rays of the trace fuzz on all faces and again on the moving ones, (d) plain random rays.  Returns o, d, aim (the face of an (a) ray, -1 else)."""
    import fuzz_trace as F
    rs = np.random.RandomState(seed)
    oa, da, aim = aimed_rays(rs, v, f, huge, AIMED_PER_FACE)
    ob, db = F.grazing_rays(rs, v, f, N_GRAZING)
    os_, ds = skimming_rays(rs, v, f, static_huge, 1e-5 * extent_measure(v), N_SKIMMING)
    oc, dc = F.rays(rs, v, f, N_FUZZ)
    om, dm = F.rays(rs, v, f[moving], N_FUZZ_MOVING)         # ... and of the moving faces alone: corners and edges of refit leaves
    lo, hi = v.min(0) - 5.0, v.max(0) + 5.0
    od = rs.uniform(lo, hi, (N_RANDOM, 3)).astype(np.float32)
    dd = rs.normal(0, 1, (N_RANDOM, 3)); dd = (dd / np.linalg.norm(dd, axis=1, keepdims=True)).astype(np.float32)
    o, d = np.concatenate([oa, ob, os_, oc, om, od]), np.concatenate([da, db, ds, dc, dm, dd])
    aim = np.concatenate([aim.astype(np.int64), np.full(len(o) - len(aim), -1, np.int64)])
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32), aim


def brute_force(oracle, v, f, o, d):
    """the oracle's loop over all triangles, one call per ray: t (f32, -1 for a miss) and face (0xFFFFFFFF for a miss)"""
    brute = oracle.Scene(v, f, None, use_bvh=0)
    t = np.full(len(o), -1.0, np.float32); face = np.full(len(o), 0xFFFFFFFF, np.uint32)
    for i in range(len(o)):
        r = brute.intersect(o[i], d[i])
        if r is not None:
            t[i], face[i] = r[0], r[1]
    return t, face


_SCENE = None
_CACHE = {}


def scene():
    global _SCENE
    if _SCENE is None:
        _SCENE = split_scene()
    return _SCENE


def state(oracle, name):
    """one state of the scene: its poses, rest vertices, posed soup, rays and the brute-force answer for them (read-only)"""
    if name not in _CACHE:
        s = scene()
        pose_name, bent = STATES[name]
        P = poses_of(pose_name)
        rest = deformed_verts(s) if bent else s["verts"]
        soup = posed_soup(s, P, verts=rest)
        o, d, aim = probe_rays(1000 + sorted(STATES).index(name), soup["verts"], soup["faces"], s["huge"], s["face_object_id"] != 0,
                             s["huge"][:s["n_static_huge"]])
        t, face = brute_force(oracle, soup["verts"], soup["faces"], o, d)
        st = {"name": name, "poses": P, "rest": rest, "soup_verts": soup["verts"], "soup_faces": soup["faces"],
              "o": o, "d": d, "aim": aim, "t": t, "face": face}
        for a in st.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[name] = st
    return _CACHE[name]
