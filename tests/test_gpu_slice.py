"""Mesh maps on the GPU (rr_slice.hip) against the numpy restatement of their definition (tests/slice_ref.py), byte for byte and on guarded
buffers: single triangles at band edges, cell corners and grid sides, degenerate and huge ones; degenerate, tile-edge and odd grids; the
boundary between the record's own thread and the large list, the prefilter's worst case and more list entries than workgroups; record
counts at the workgroup's edges; a scene that both tree builders cut; posed, deformed and rebuilt scenes against a fresh context; the skip
list and the object plane; accumulation; every refusal, with the outputs untouched; covering and tightness of a device result; a call on a
second stream beside a batch in flight; a closed loop through the simulator; and the C++ driver."""
import math
import os
import subprocess

import numpy as np
import pytest

import dynamic_ref as D
import field_ref as F
import icp_ref
import slice_ref as R
from common import golden_beams
from radarays_ros_amd import native, params, radar

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
GUARD = 0xA5


@pytest.fixture(scope="module")
def ctx():
    return native.Context(0)


@pytest.fixture(scope="module")
def cases():
    return R.all_cases(*native.slice_tile_sizes())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)


def guarded(payload_bytes):
    """the payload as given, 64 guard bytes behind it"""
    raw = dev(payload_bytes)
    t = torch.full((len(raw) + 64,), GUARD, dtype=torch.uint8, device=DEV)
    t[:len(raw)] = raw
    return t


def payload(t, n_bytes):
    raw = t.cpu().numpy()
    assert np.all(raw[n_bytes:] == GUARD)                             # nothing behind the buffer
    return raw[:n_bytes].copy()


def load(c, soup, obj, builder="host"):
    soup = np.ascontiguousarray(soup, np.float32).reshape(-1, 3, 3)
    c.set_mesh(soup.reshape(-1, 3), np.arange(3 * len(soup), dtype=np.uint32).reshape(-1, 3), np.ascontiguousarray(obj, np.uint32), builder=builder)


def run(c, band, g, skip=None, occ=None, objects=None, with_objects=True, stream=None):
    """rr_slice_mesh_device on guarded buffers -> (occ uint8 [height][width], objects uint32 [height][width] or None)"""
    g = native._field_cfg(g)
    cells = g.width * g.height
    d_occ = guarded(np.zeros(cells, np.uint8) if occ is None else np.ascontiguousarray(occ, np.uint8).reshape(-1))
    d_obj = None
    if with_objects:
        d_obj = guarded(np.full(cells, R.OBJECT_NONE, np.uint32) if objects is None else np.ascontiguousarray(objects, np.uint32).reshape(-1))
    d_skip = None if skip is None else dev(np.ascontiguousarray(skip, np.uint8))
    torch.cuda.synchronize()
    c.slice_mesh_device(band, g, d_occ.data_ptr(), None if d_obj is None else d_obj.data_ptr(), None if d_skip is None else d_skip.data_ptr(), stream)
    torch.cuda.synchronize()
    c.synchronize()
    got = payload(d_occ, cells).reshape(g.height, g.width)
    ids = None if d_obj is None else payload(d_obj, 4 * cells).view(np.uint32).reshape(g.height, g.width)
    return got, ids


def check_case(c, case):
    load(c, case["soup"], case["obj"])
    want, want_ids = R.slice_mesh(case["soup"], case["obj"], case["skip"], case["band"], case["grid"])
    got, ids = run(c, case["band"], case["grid"], case["skip"])
    assert np.array_equal(got, want), (case["label"], np.argwhere(got != want)[:6], int(got.sum()), int(want.sum()))
    assert np.array_equal(ids, want_ids), (case["label"], np.argwhere(ids != want_ids)[:6])
    return int(want.sum())


# ---- 1. the shared cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["single", "grid", "box", "diagonal", "long", "records"])
def test_device_maps_equal_the_restatement(ctx, cases, kind):
    mine = [c for c in cases if c["label"][0] == kind]
    assert mine
    marked = [check_case(ctx, c) for c in mine]
    if kind != "single":
        assert all(m > 0 for m in marked), marked
    else:
        assert sum(1 for m in marked if m == 0) == 8 and sum(1 for m in marked if m > 0) >= 20


def test_an_empty_mesh_writes_nothing(ctx):
    ctx.set_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32))
    pre = np.arange(12 * 10, dtype=np.uint8).reshape(10, 12)
    got, ids = run(ctx, (0.0, 1.0), R.grid(12, 10), occ=pre)
    assert np.array_equal(got, pre) and np.all(ids == R.OBJECT_NONE)
    assert np.array_equal(ctx.slice_mesh((0.0, 1.0), R.grid(12, 10), occ=pre), pre)


# ---- 2. a scene that both builders cut, and its dynamic states ---------------------------------------------------------------------------------
SPLIT_GRID = native.field_config(84, 84, 0.5, -21.0, -21.0, 8, 0)
SPLIT_BAND = (0.0, 0.6)


def soup_of(scene):
    return scene["verts"][scene["faces"].reshape(-1)].reshape(-1, 3, 3).astype(np.float32)


def moved_poses():
    p = D.identity_poses(D.N_OBJECTS)
    p[1] = D.about((0.0, 0.0, 0.0), 0.3, (0.4, -0.2, 0.1))
    p[2] = D.about((2.0, 1.0, 0.0), -0.7, (1.5, 0.5, 0.2))
    p[3] = D.about((0.0, 0.0, 0.0), 1.1, (-3.0, 2.0, 0.3))
    p[4] = D.about((0.0, 0.0, 0.0), 0.0, (0.0, 0.0, 0.25))
    return p


@pytest.fixture(scope="module")
def split_want():
    s = D.split_scene()
    return s, R.slice_mesh(soup_of(s), s["face_object_id"], None, SPLIT_BAND, SPLIT_GRID)


@pytest.mark.parametrize("builder", ["host", "gpu"])
def test_records_of_split_faces_are_harmless(split_want, builder):
    s, (want, want_ids) = split_want
    c = native.Context(0)
    c.set_mesh(s["verts"], s["faces"], s["face_object_id"], builder=builder)
    assert c.bvh_info()["n_tris"] > len(s["faces"])                   # the builder did cut faces: several records per face
    got, ids = run(c, SPLIT_BAND, SPLIT_GRID)
    assert np.array_equal(got, want) and np.array_equal(ids, want_ids) and want.sum() > 500
    c.close()


def test_posed_deformed_and_rebuilt_scenes_equal_a_fresh_context_of_the_posed_soup(split_want):
    s, (want0, _) = split_want
    c, fresh = native.Context(0), native.Context(0)
    c.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    poses = moved_poses()
    c.set_object_poses(poses)
    posed = D.posed_soup(s, poses)
    fresh.set_mesh(posed["verts"], posed["faces"], s["face_object_id"])
    a, a_ids = run(c, SPLIT_BAND, SPLIT_GRID)
    b, b_ids = run(fresh, SPLIT_BAND, SPLIT_GRID)
    want, want_ids = R.slice_mesh(soup_of(posed), s["face_object_id"], None, SPLIT_BAND, SPLIT_GRID)
    assert np.array_equal(a, b) and np.array_equal(a_ids, b_ids) and np.array_equal(a, want) and np.array_equal(a_ids, want_ids)
    assert not np.array_equal(a, want0)                               # the poses did move something in the band
    # new rest vertices: the terrain deformed, the poses kept
    rest = s["verts"].copy()
    rest[:D.N_TERRAIN_VERTS, 2] += np.random.RandomState(4).uniform(-0.3, 0.3, D.N_TERRAIN_VERTS).astype(np.float32)
    c.update_vertices(rest)
    deformed = D.posed_soup(s, poses, rest)
    fresh.set_mesh(deformed["verts"], deformed["faces"], s["face_object_id"])
    a2, a2_ids = run(c, SPLIT_BAND, SPLIT_GRID)
    b2, b2_ids = run(fresh, SPLIT_BAND, SPLIT_GRID)
    assert np.array_equal(a2, b2) and np.array_equal(a2_ids, b2_ids) and not np.array_equal(a2, a)
    for builder in ("host", "gpu"):
        c.rebuild_tree(builder)
        a3, a3_ids = run(c, SPLIT_BAND, SPLIT_GRID)
        assert np.array_equal(a3, b2) and np.array_equal(a3_ids, b2_ids), builder
    c.close()
    fresh.close()


# ---- 3. skip list, object plane, accumulation --------------------------------------------------------------------------------------------------
def test_skip_list_and_object_plane(split_want):
    s, (want, want_ids) = split_want
    c = native.Context(0)
    c.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    oid = s["face_object_id"]
    skip = np.zeros(D.N_OBJECTS, np.uint8)
    skip[[1, 2]] = 1
    keep = ~np.isin(oid, [1, 2])
    without, without_ids = R.slice_mesh(soup_of(s)[keep], oid[keep], None, SPLIT_BAND, SPLIT_GRID)
    got, ids = run(c, SPLIT_BAND, SPLIT_GRID, skip)
    assert np.array_equal(got, without) and np.array_equal(ids, without_ids) and without.sum() < want.sum()
    assert not np.isin(ids, [1, 2]).any() and np.array_equal(ids == R.OBJECT_NONE, got == 0)
    # overlapping objects: a cell takes the smallest id, whatever the plane held above it; a lower id it held stays
    pre = np.full((SPLIT_GRID.height, SPLIT_GRID.width), 3, np.uint32)
    _, low = run(c, SPLIT_BAND, SPLIT_GRID, objects=pre)
    assert np.array_equal(low, np.minimum(want_ids, 3))
    assert (want_ids == 0).sum() > 100 and (want_ids == 1).sum() > 0 and int(want_ids.max()) == R.OBJECT_NONE
    # the wrapper's skip list, and no object plane at all
    assert np.array_equal(c.slice_mesh(SPLIT_BAND, SPLIT_GRID, skip_objects=[1, 2]), without)
    only, none = run(c, SPLIT_BAND, SPLIT_GRID, with_objects=False)
    assert none is None and np.array_equal(only, want)
    c.close()


def test_accumulation_bands_and_the_host_form(split_want):
    s, (want, want_ids) = split_want
    c = native.Context(0)
    c.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    rs = np.random.RandomState(12)
    pre = rs.choice(np.array([0, 1, 7, 200, 255], np.uint8), want.shape, p=[0.9, 0.025, 0.025, 0.025, 0.025])
    got, _ = run(c, SPLIT_BAND, SPLIT_GRID, occ=pre)
    assert np.array_equal(got, np.where(want == 1, 1, pre)) and (got == 200).any()           # ones only, nothing cleared
    upper = (1.0, 2.5)
    high, _ = R.slice_mesh(soup_of(s), s["face_object_id"], None, upper, SPLIT_GRID)
    one, _ = run(c, upper, SPLIT_GRID)
    two, _ = run(c, SPLIT_BAND, SPLIT_GRID, occ=one)
    assert np.array_equal(one, high) and np.array_equal(two, want | high) and not np.array_equal(high, want)
    rev, _ = run(c, upper, SPLIT_GRID, occ=want)                                             # the other order
    assert np.array_equal(rev, two)
    # the host form equals the device form, with and without the plane, accumulating like it
    h_occ, h_ids = c.slice_mesh(SPLIT_BAND, SPLIT_GRID, with_objects=True)
    assert np.array_equal(h_occ, want) and np.array_equal(h_ids, want_ids)
    assert np.array_equal(c.slice_mesh(upper, SPLIT_GRID, occ=want), two)
    h2_occ, h2_ids = c.slice_mesh(SPLIT_BAND, SPLIT_GRID, objects=np.full(want.shape, 3, np.uint32))
    assert np.array_equal(h2_ids, np.minimum(want_ids, 3)) and np.array_equal(h2_occ, want)
    c.close()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ctx):
    load(ctx, R.xyz([[[1.5, 1.5, 0.5], [6.5, 1.5, 0.5], [1.5, 6.5, 0.5]]], R.grid(8, 8)), [0])
    L, h = ctx._L, ctx._h
    d = torch.full((4096,), GUARD, dtype=torch.uint8, device=DEV)
    occ, obj = d.data_ptr(), d.data_ptr() + 1024
    import ctypes as C
    cfg = lambda **kw: C.byref(native.RRFieldConfig(**dict(dict(width=8, height=8, cell=0.5, x0=0.0, y0=0.0, max_dist=4, gate=1, reserved_=0), **kw)))   # noqa: E731
    band = lambda lo=0.0, hi=1.0, flags=0: C.byref(native.RRSliceConfig(lo, hi, flags, 0))                                                            # noqa: E731
    call = lambda b=None, g=None, o=occ, ids=obj: L.rr_slice_mesh_device(h, b or band(), g or cfg(), None, o, ids, None)                              # noqa: E731
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((d[:64] != GUARD).any())                              # (the call does write when it is taken)
    d.fill_(GUARD)
    torch.cuda.synchronize()
    assert L.rr_slice_mesh_device(None, band(), cfg(), None, occ, obj, None) == -1
    bare = native.Context(0)
    assert bare._L.rr_slice_mesh_device(bare._h, band(), cfg(), None, occ, obj, None) == -2 and b"rr_set_mesh" in L.rr_last_error(bare._h)
    nan, inf = float("nan"), float("inf")
    for b in (band(1.0, 0.5), band(nan, 1.0), band(0.0, nan), band(-inf, 1.0), band(0.0, inf), band(flags=1), band(flags=0x80000000)):
        assert call(b=b) == -3 and b"rr_slice_mesh_device" in L.rr_last_error(h)
    for kw in (dict(width=0), dict(width=4097), dict(height=0), dict(height=4097), dict(cell=0.0), dict(cell=-0.5), dict(cell=nan), dict(cell=inf),
               dict(x0=nan), dict(y0=-inf), dict(max_dist=0), dict(max_dist=256), dict(gate=-1), dict(gate=5)):
        assert call(g=cfg(**kw)) == -3, kw
    assert call(o=None) == -3 and call(ids=obj + 2) == -3 and call(ids=obj + 1) == -3
    assert L.rr_slice_mesh_device(h, None, cfg(), None, occ, obj, None) == -3 and L.rr_slice_mesh_device(h, band(), None, None, occ, obj, None) == -3
    torch.cuda.synchronize()
    assert bool((d == GUARD).all())
    # the host form, on host buffers pre-filled with a pattern
    h_occ, h_obj = np.full((8, 8), GUARD, np.uint8), np.full((8, 8), GUARD * 0x01010101, np.uint32)
    host = lambda b=None, g=None, o=h_occ.ctypes.data, ids=h_obj.ctypes.data, who=h: L.rr_slice_mesh(who, b or band(), g or cfg(), None, o, ids)     # noqa: E731
    assert L.rr_slice_mesh(None, band(), cfg(), None, h_occ.ctypes.data, h_obj.ctypes.data) == -1
    assert host(who=bare._h) == -2
    for kw in (dict(b=band(1.0, 0.5)), dict(b=band(nan, 0.0)), dict(b=band(flags=2)), dict(g=cfg(width=0)), dict(g=cfg(cell=nan)), dict(g=cfg(gate=9)),
               dict(o=None), dict(ids=h_obj.ctypes.data + 2)):
        assert host(**kw) == -3 and b"rr_slice_mesh" in L.rr_last_error(h), kw
    assert np.all(h_occ == GUARD) and np.all(h_obj == GUARD * 0x01010101)
    bare.close()


# ---- 5. covering and tightness of a device result ------------------------------------------------------------------------------------------------
def test_covering_and_tightness_of_a_device_result(ctx, cases):
    (case,) = [c for c in cases if c["label"] == ("grid", 257, 130)]
    load(ctx, case["soup"], case["obj"])
    got, _ = run(ctx, case["band"], case["grid"])
    n, missed = R.covering(got, case)
    m, loose = R.tightness(got, case)
    assert n > 1000 and missed == 0 and m > 1000 and loose == 0, (n, missed, m, loose)


# ---- 6. two streams -------------------------------------------------------------------------------------------------------------------------------
def loop_context():
    s, cfg = icp_ref.loop_scene(), icp_ref.loop_cfg()
    c = native.Context(0)
    c.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    c.set_materials(params.kaist_materials(), s["object_materials"], 0)
    c.set_config(cfg, icp_ref.LOOP_ANGLES)
    c.set_beam_samples(golden_beams(icp_ref.LOOP_SAMPLES))
    return c, cfg


def test_slicing_on_a_second_stream_beside_a_batch_in_flight():
    c, rcfg = loop_context()
    g = F.loop_field_cfg()
    cells = g.width * g.height
    soup, obj = R.loop_soup()
    want, want_ids = R.slice_mesh(soup, obj, None, R.LOOP_BAND, g)
    poses = np.stack([icp_ref.loop_pose((0.1 * k, 0.05 * k, 0.01 * k)) for k in range(8)])
    imgs = torch.zeros((8, rcfg.n_cells, icp_ref.LOOP_ANGLES), dtype=torch.uint8, device=DEV)
    d_occ = torch.zeros(cells, dtype=torch.uint8, device=DEV)
    d_obj = torch.full((cells,), -1, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    c.simulate_batch_device(poses, imgs.data_ptr(), None)             # a batch in flight on the context's stream
    c.slice_mesh_device(R.LOOP_BAND, g, d_occ.data_ptr(), d_obj.data_ptr(), None, side.cuda_stream)
    torch.cuda.synchronize()
    c.synchronize()
    beside = d_occ.cpu().numpy().reshape(g.height, g.width)
    beside_ids = d_obj.cpu().numpy().view(np.uint32).reshape(g.height, g.width)
    busy = imgs.cpu().numpy().copy()
    assert np.array_equal(beside, want) and np.array_equal(beside_ids, want_ids) and want.sum() > 100
    alone, alone_ids = run(c, R.LOOP_BAND, g)                         # alone, on the context's stream
    assert np.array_equal(alone, want) and np.array_equal(alone_ids, want_ids)
    imgs.zero_()
    torch.cuda.synchronize()
    c.simulate_batch_device(poses, imgs.data_ptr(), None)
    c.synchronize()
    assert np.array_equal(imgs.cpu().numpy(), busy) and busy.any()   # ... and the batch beside it was not disturbed
    c.close()


# ---- 7. closed loop ---------------------------------------------------------------------------------------------------------------------------------
def test_closed_loop_a_scan_is_localised_in_the_map_of_the_mesh():
    s = icp_ref.loop_scene()
    r = radar.RadarHIP(s["verts"], s["faces"], s["face_object_id"])
    r.loadParams(params.kaist_materials(), s["object_materials"], 0)
    r.updateDynCfg(icp_ref.loop_cfg())
    r.setBeamSamples(golden_beams(icp_ref.LOOP_SAMPLES))
    cfg = F.loop_field_cfg()
    occ, ids = r.buildMeshMap(cfg, *R.LOOP_BAND, with_objects=True)
    soup, obj = R.loop_soup()
    want, want_ids = R.slice_mesh(soup, obj, None, R.LOOP_BAND, cfg)
    assert occ.dtype == np.uint8 and np.array_equal(occ, want) and np.array_equal(ids, want_ids)
    assert np.array_equal(r.buildMeshMap(cfg, *R.LOOP_BAND, skip_objects=[0]), np.zeros_like(want))      # the room is one object
    c, _ = loop_context()
    img = c.simulate(icp_ref.loop_pose(icp_ref.LOOP_B))[0]
    pts, offs = c.detect(img[None], icp_ref.LOOP_DET)
    assert len(pts[0]) >= 100
    fld = c.distance_field(occ, cfg)
    assert np.array_equal(fld, F.distance_field(occ, cfg))
    states, xyz = F.loop_lattice()
    rec = c.score_poses(pts[0], states, fld, cfg)
    best, centre = int(np.argmin(rec["sum_d2"])), len(states) // 2
    ex, ey, eyaw = F.loop_errors(xyz[best])
    print("closed loop on the GPU: argmin node (%.2f m, %.2f m, %.1f deg) at sum_d2 %d (centre node %d), off the truth by %.3f m, %.3f m, %.3f deg"
          % (xyz[best][0], xyz[best][1], math.degrees(xyz[best][2]), rec["sum_d2"][best], rec["sum_d2"][centre], ex, ey, math.degrees(eyaw)))
    # within the figure measured on the oracle's image plus one lattice step in each of x, y and yaw
    assert ex <= R.LOOP_X_MEASURED + F.LOOP_STEP_XY + 1e-9 and ey <= R.LOOP_Y_MEASURED + F.LOOP_STEP_XY + 1e-9
    assert eyaw <= R.LOOP_YAW_MEASURED + F.LOOP_STEP_YAW + 1e-9
    assert rec["sum_d2"][best] < rec["sum_d2"][centre]
    c.close()


# ---- 8. the C++ mirror ------------------------------------------------------------------------------------------------------------------------------
def test_cpp_build_mesh_map_equals_the_ctypes_path(tmp_path):
    native.build()
    exe = str(tmp_path / "slice_check")
    lib_dir = os.path.join(ROOT, "radarays_ros_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "slice_check.cpp"), "-o", exe, "-L", lib_dir, "-lradarays_mi355", "-Wl,-rpath," + lib_dir],
                   check=True)
    g = R.grid(40, 30)
    rs = np.random.RandomState(31)
    soup = np.concatenate([R._random_soup(rs, 60, g, 1.5), R._random_soup(rs, 6, g, 12.0)])
    oid = (np.arange(len(soup)) % 4).astype(np.uint32)
    verts, faces = soup.reshape(-1, 3), np.arange(3 * len(soup), dtype=np.uint32)
    first, second, skip = (0.0, 1.0), (1.0, 2.0), np.array([1, 3], np.uint32)
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.int32([len(verts), len(soup), g.width, g.height, len(skip)]).tobytes())
        f.write(np.float32([g.cell, g.x0, g.y0, first[0], first[1], second[0], second[1]]).tobytes())
        f.write(verts.tobytes() + faces.tobytes() + oid.tobytes() + skip.tobytes())
    p = subprocess.run([exe, str(inp), str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    raw = open(out, "rb").read()
    cells = g.width * g.height
    assert len(raw) == cells * 6
    cpp_first = np.frombuffer(raw[:cells], np.uint8).reshape(g.height, g.width)
    cpp_ids = np.frombuffer(raw[cells:5 * cells], np.uint32).reshape(g.height, g.width)
    cpp_both = np.frombuffer(raw[5 * cells:], np.uint8).reshape(g.height, g.width)
    c = native.Context(0)
    load(c, soup, oid)
    occ, ids = c.slice_mesh(first, g, skip_objects=skip.tolist(), with_objects=True)
    both = c.slice_mesh(first, g, occ=c.slice_mesh(second, g))
    assert cpp_first.tobytes() == occ.tobytes() and cpp_ids.tobytes() == ids.tobytes() and cpp_both.tobytes() == both.tobytes()
    assert occ.any() and both.sum() > occ.sum()                       # not vacuous: the first band marks cells, the second adds some
    sk = np.zeros(4, np.uint8)
    sk[skip] = 1
    assert np.array_equal(occ, R.slice_mesh(soup, oid, sk, first, g)[0])
    c.close()
