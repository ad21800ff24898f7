"""The pop of the stack walk (traverse(), rr_kernels.hip): the culling walk reads its first pop candidate beside the step's
loads and pops it from registers.  What can go wrong is the pop: a stale or wrong entry, a read below the stack, the
boundary between the LDS stack and the spill buffer.

  * generic rays that start on surfaces (as later-pass rays do) against the oracle's brute-force nearest hit, bit for bit,
    cull on and off, at the default LDS depth and at the smallest one (RR_STACK_LDS=1: every pop but the last crosses
    the LDS / spill boundary, pops at sp - 1 == stack_lds and at stack_lds - 1 right after included)
  * a frame chain of 2 poses x 12 azimuths x 24 rays x 3 passes in a closed room with a penetrable box (the CULL,
    non-spill instantiation bench.py runs): images and statistics against the oracle
  * one ray on a one-leaf tree: sp == 0 at the top of every iteration
"""
import numpy as np
import pytest

from common import golden_beams, mats_tuple
from radarays_ros_amd import params, scenes

pytestmark = pytest.mark.gpu

N_TRIS, N_RAYS = 3000, 2500
_cache = {}


def _soup():
    rs = np.random.RandomState(21)
    cen = rs.uniform(-30, 30, (N_TRIS, 1, 3))
    v = (cen + rs.normal(0, 2.0, (N_TRIS, 3, 3))).astype(np.float32).reshape(-1, 3)
    f = np.arange(3 * N_TRIS, dtype=np.uint32).reshape(N_TRIS, 3)
    return v, f


def _surface_rays(native_lib, oracle):
    """(verts, faces, origins, directions, brute-force t, brute-force face): computed once, never modified"""
    if "rays" not in _cache:
        v, f = _soup()
        rs = np.random.RandomState(22)
        o0 = rs.uniform(-35, 35, (4 * N_RAYS, 3)).astype(np.float32)
        d0 = rs.normal(0, 1, (4 * N_RAYS, 3))
        d0 = (d0 / np.linalg.norm(d0, axis=1, keepdims=True)).astype(np.float32)
        c = native_lib.Context(0)
        c.set_mesh(v, f)
        t0, _ = c.debug_trace(o0, d0)
        c.close()
        on = np.flatnonzero(t0 > 0)[:N_RAYS]
        assert len(on) == N_RAYS
        o = (o0[on] + t0[on, None] * d0[on]).astype(np.float32)          # on (within rounding of) a triangle
        d = rs.normal(0, 1, (N_RAYS, 3))
        d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        brute = oracle.Scene(v, f, None, use_bvh=0)
        bt = np.full(N_RAYS, -1.0, np.float32)
        bf = np.zeros(N_RAYS, np.uint32)
        for i in range(N_RAYS):
            r = brute.intersect(o[i], d[i])
            if r is not None:
                bt[i], bf[i] = np.float32(r[0]), r[1]
        for a in (o, d, bt, bf):
            a.setflags(write=False)
        _cache["rays"] = (v, f, o, d, bt, bf)
    return _cache["rays"]


@pytest.mark.parametrize("cull", ["1", "0"], ids=["cull", "nocull"])
@pytest.mark.parametrize("lds", [None, "1"], ids=["lds-default", "lds-1"])
def test_surface_rays_equal_brute_force(native_lib, oracle, monkeypatch, lds, cull):
    v, f, o, d, bt, bf = _surface_rays(native_lib, oracle)
    monkeypatch.setenv("RR_CULL_POP", cull)
    if lds is not None:
        monkeypatch.setenv("RR_STACK_LDS", lds)
    c = native_lib.Context(0)
    c.set_mesh(v, f)
    assert c.bvh_info()["stack_need"] > 3            # deeper than the shallow LDS stack: pops cross the boundary both ways
    t, face = c.debug_trace(o, d)
    c.close()
    hit = bt >= 0
    assert 500 < hit.sum() < N_RAYS                  # hits and misses (a miss ends with sp == 0 at the pop)
    assert np.array_equal(t < 0, ~hit), np.flatnonzero((t < 0) != ~hit)[:8]
    assert np.array_equal(t[hit].view(np.uint32), bt[hit].view(np.uint32)), np.flatnonzero(hit)[t[hit] != bt[hit]][:8]
    assert np.array_equal(face[hit], bf[hit]), np.flatnonzero(hit)[face[hit] != bf[hit]][:8]


def test_frame_chain_with_a_penetrable_box(native_lib, oracle):
    import torch
    n_az, n_beam = 12, 24
    room = scenes.box12()
    bv, bfa = scenes._box_tris([2.0, -3.0, -0.5], [5.0, 2.5, 2.5], vbase=len(room["verts"]))
    s = {"verts": np.concatenate([room["verts"], bv]), "faces": np.concatenate([room["faces"], bfa]),
         "face_object_id": np.concatenate([room["face_object_id"], np.ones(12, np.uint32)]), "object_materials": [1, 2]}
    mats = params.kaist_materials() + [params.PENETRABLE]
    cfg = params.kaist_preset(n_reflections=3, ambient_noise=0)
    beams = golden_beams(n_beam)
    poses = np.stack([scenes.yaw_pose(-1.0, 0.5, 0.4, 0.3), scenes.yaw_pose(-4.0, -2.0, 1.0, -1.2)])
    c = native_lib.Context(0)
    c.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    c.set_materials(mats, s["object_materials"], 0)
    c.set_config(cfg, n_az)
    c.set_beam_samples(beams)
    imgs = torch.zeros((2, cfg.n_cells, n_az), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    sp = torch.cuda.current_stream().cuda_stream
    c.simulate_batch_device(poses, imgs.data_ptr(), sp)
    c.synchronize(sp)
    gst = c.stats()
    got = imgs.cpu().numpy()
    c.close()
    sc = oracle.Scene(s["verts"], s["faces"], s["face_object_id"], use_bvh=0)
    tot = {"wave_passes": 0, "hits": 0, "signals": 0}
    for k, p in enumerate(poses):
        o8, _, ost = oracle.simulate(sc, mats_tuple(mats), s["object_materials"], cfg, beams, p, n_angles=n_az, want_f32=False)
        assert o8.any()
        assert np.array_equal(got[k], o8), (k, np.argwhere(got[k] != o8)[:8])
        for key in tot:
            tot[key] += ost[key]
    assert gst["overflow"] == 0
    assert {key: gst[key] for key in tot} == tot
    assert tot["wave_passes"] > 2 * n_az * n_beam                       # later passes ran


@pytest.mark.parametrize("cull", ["1", "0"], ids=["cull", "nocull"])
def test_single_ray_on_a_single_leaf_tree(native_lib, oracle, monkeypatch, cull):
    monkeypatch.setenv("RR_CULL_POP", cull)
    v = np.float32([[0, 0, 5], [1, 0, 5], [0, 1, 5]])
    f = np.uint32([[0, 1, 2]])
    c = native_lib.Context(0)
    c.set_mesh(v, f)
    o, d = np.float32([[0.2, 0.2, 0]]), np.float32([[0, 0, 1]])
    t, face = c.debug_trace(o, d)
    tm, _ = c.debug_trace(o, -d)
    c.close()
    r = oracle.Scene(v, f, None, use_bvh=0).intersect(o[0], d[0])
    assert r is not None and t[0] == np.float32(r[0]) and face[0] == r[1]
    assert tm[0] < 0
