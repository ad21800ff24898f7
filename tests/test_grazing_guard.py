"""The grazing guard of the triangle test (round 5; oracle/radarays_oracle.c: tri_hit, csrc/rr_kernels.hip: leaf_step).

Round 4's nearest-hit fuzz found ONE ray in 39 M (seed 307, ray 389) on which the brute-force loop and every hierarchy
disagreed: it grazes a triangle's plane at |d . n| = 4.3e-5, Moeller-Trumbore's barycentric test accepts a point 6.4 mm
outside that triangle -- outside the padded box any hierarchy keeps the triangle in.  The hit definition is now independent
of the structure that finds it: a hit with det^2 < 2.5e-5 |e1 x e2|^2 counts only if its point lies in the triangle's
box padded by 1e-5 x the scene's extent.  This file pins the case: CPU (oracle brute force == oracle BVH2 == the
documented answer; the unguarded test, restated in numpy f32 for this one ray, gives the old one) and GPU (both tree
builders, all 3000 rays of the scene bit-exact against the oracle's brute force -- no exception class any more)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz"))

RAY, T_GUARDED, FACE_GUARDED, FACE_UNGUARDED = 389, np.float32(21.656564712524414), 1921, 1880


def _case():
    import fuzz_trace as F
    rs = np.random.RandomState(307)
    v, f = F.scene(rs)
    o, d = F.rays(rs, v, f)
    return v, f, o, d


def _mt_unguarded_f32(o, d, v0, v1, v2):
    """Moeller-Trumbore as radarays_oracle.c: tri_hit without the guard, every operation rounded to f32"""
    f = np.float32
    e1, e2 = (v1 - v0).astype(f), (v2 - v0).astype(f)

    def cross(a, b):
        return np.array([f(f(a[1] * b[2]) - f(a[2] * b[1])), f(f(a[2] * b[0]) - f(a[0] * b[2])), f(f(a[0] * b[1]) - f(a[1] * b[0]))], f)

    def dot(a, b):
        return f(f(f(a[0] * b[0]) + f(a[1] * b[1])) + f(a[2] * b[2]))
    pvec = cross(d, e2); det = dot(e1, pvec)
    inv = f(f(1.0) / det); tvec = (o - v0).astype(f)
    u = f(dot(tvec, pvec) * inv); qvec = cross(tvec, e1); vv = f(dot(d, qvec) * inv); t = f(dot(e2, qvec) * inv)
    return bool(det != 0 and 0 <= u <= 1 and vv >= 0 and f(u + vv) <= 1 and 0 < t <= 1000), t, det, e1, e2


def test_grazing_ray_on_the_cpu(oracle):
    v, f, o, d = _case()
    brute, bvh = oracle.Scene(v, f, None, use_bvh=0), oracle.Scene(v, f, None, use_bvh=1)
    for i in list(range(0, len(o), 7)) + [RAY]:                      # the brute-force loop and the BVH2 agree, ray by ray
        a, b = brute.intersect(o[i], d[i]), bvh.intersect(o[i], d[i])
        assert (a is None) == (b is None) and (a is None or (a[0] == b[0] and a[1] == b[1])), i
    t, face, _ = brute.intersect(o[RAY], d[RAY])
    assert np.float32(t) == T_GUARDED and face == FACE_GUARDED
    # what the unguarded test says about the triangle the guard rejects: a "hit", nearer, 6.4 mm outside its box
    tri = v[f[FACE_UNGUARDED]]
    hit, t_old, det, e1, e2 = _mt_unguarded_f32(o[RAY], d[RAY], tri[0], tri[1], tri[2])
    assert hit and t_old < T_GUARDED
    n = np.cross(e1.astype(np.float64), e2.astype(np.float64)); area2 = np.linalg.norm(n); n /= area2
    assert abs(float(n @ d[RAY].astype(np.float64))) < 2e-4                                   # grazing: 4.3e-5
    assert float(det) ** 2 < 2.5e-5 * area2 ** 2                                              # ... so the guard looks at it
    pt = o[RAY].astype(np.float64) + float(t_old) * d[RAY].astype(np.float64)
    outside = np.maximum(np.maximum(tri.min(0) - pt, pt - tri.max(0)), 0.0).max()
    ext = max((v.max(0) - v.min(0)).max(), np.abs(v).max())
    assert outside > 1e-3 and outside > 1e-5 * ext                                            # 6.4 mm against a 0.4 mm pad
    # the triangle the guarded test returns is an ordinary hit
    tri2 = v[f[FACE_GUARDED]]
    hit2, t_new, det2, a1, a2 = _mt_unguarded_f32(o[RAY], d[RAY], tri2[0], tri2[1], tri2[2])
    assert hit2 and t_new == T_GUARDED


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "gpu"])
def test_grazing_ray_on_the_gpu(native_lib, oracle, builder):
    v, f, o, d = _case()
    brute = oracle.Scene(v, f, None, use_bvh=0)
    want_t = np.full(len(o), -1.0, np.float32); want_f = np.full(len(o), 0xFFFFFFFF, np.uint32)
    for i in range(len(o)):
        r = brute.intersect(o[i], d[i])
        if r is not None:
            want_t[i], want_f[i] = r[0], r[1]
    c = native_lib.Context(0)
    c.set_mesh(v, f, None, builder=builder)
    t, face = c.debug_trace(o, d)
    c.close()
    hit = want_t >= 0
    assert np.array_equal(t[hit], want_t[hit]) and np.array_equal(face[hit], want_f[hit]) and (t[~hit] < 0).all()
    assert t[RAY] == T_GUARDED and face[RAY] == FACE_GUARDED
