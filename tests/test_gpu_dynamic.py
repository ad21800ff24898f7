"""Dynamic scenes on the GPU: per-object rigid poses and new rest vertices, the tree refit in place (rr_refit.hip).

The oracle for every case is free: the nearest hit does not depend on the tree, so a refit context must render exactly
what a FRESH context renders when it is given the posed triangle soup (every face's rest corners moved by its object's
pose, same face order and ids), built here in numpy float32 with the library's op order.  The soup is also checked against
the CPU oracle with the parity tolerances of tests/test_gpu_parity.py."""
import numpy as np
import pytest

from common import golden_beams, image_diff, materials_for, mats_tuple
from dynamic_ref import about, identity_poses, posed_soup
from radarays_ros_amd import params, scenes

pytestmark = pytest.mark.gpu

MEAN_DEV_TOL = 1e-5
U8_MISMATCH_TOL = 1e-3


# ---- contexts ---------------------------------------------------------------------------------------------------------
def make_ctx(native_lib, scene, mats, objmat, cfg, beams, builder="host"):
    c = native_lib.Context(0)
    c.set_mesh(scene["verts"], scene["faces"], scene["face_object_id"], builder=builder)
    c.set_materials(mats, objmat, 0)
    c.set_config(cfg)
    c.set_beam_samples(beams)
    return c


def frame(c, pose):
    g8, gf, st = c.simulate(pose, want_f32=True)
    assert st["overflow"] == 0
    return g8, gf, st


def assert_same(a, b):
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    for k in ("wave_passes", "hits", "signals"):
        assert a[2][k] == b[2][k], (k, a[2], b[2])


def fresh_frame(native_lib, soup, mats, objmat, cfg, beams, pose, builder="host"):
    c = make_ctx(native_lib, soup, mats, objmat, cfg, beams, builder)
    r = frame(c, pose)
    c.close()
    return r


def oracle_parity(oracle, soup, mats, objmat, cfg, beams, pose, got):
    sc = oracle.Scene(soup["verts"], soup["faces"], soup["face_object_id"], use_bvh=0)
    o8, of, ost = oracle.simulate(sc, mats_tuple(mats), objmat, cfg, beams, pose)
    g8, gf, gst = got
    assert gst["wave_passes"] == ost["wave_passes"] and gst["hits"] == ost["hits"] and gst["signals"] == ost["signals"]
    d = image_diff(gf, of, g8, o8)
    assert d["mean_dev"] <= MEAN_DEV_TOL and d["u8_max"] <= 1 and d["u8_mismatch_frac"] <= U8_MISMATCH_TOL, d


def oru4_setup(table="oru4_test"):
    s = scenes.oru4_like_scene()
    mats = {"oru4_test": params.oru4_test_materials, "oru4_legacy": params.oru4_legacy_materials}[table]()
    cfg = params.kaist_preset(ambient_noise=0, n_samples=40)
    return s, mats, params.ORU4_OBJECT_MATERIALS, cfg, golden_beams(40), scenes.default_pose(s["name"])


def doors_open(s, frac=1.0):
    """every door leaf turned about its hinge (its low-x edge), the first locker shifted along the hallway"""
    names = s["object_names"]
    P = identity_poses(len(names))
    for oid, n in enumerate(names):
        sel = s["verts"][np.unique(s["faces"][s["face_object_id"] == oid])]
        if n.startswith("Door") and n != "DoorHallway1Glass":
            hinge = (sel[:, 0].min(), sel[:, 1].mean(), 0.0)
            P[oid] = about(hinge, frac * (-1.2 if "Lab" in n else 1.2))
        elif n == "DoorHallway1Glass":
            P[oid] = about((12.0, 0.0, 0.0), frac * 0.9)
        elif n == "Locker":
            P[oid] = about(sel.mean(0), 0.0, (frac * -1.5, 0.8 * frac, 0.0))
    return P


# ---- 1. identity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["host", "gpu"])
def test_identity_updates_change_nothing(native_lib, builder):
    s, mats, objmat, cfg, beams, pose = oru4_setup()
    c = make_ctx(native_lib, s, mats, objmat, cfg, beams, builder)
    before = frame(c, pose)
    c.update_vertices(s["verts"])
    assert_same(frame(c, pose), before)
    c.set_object_poses(identity_poses(18))
    assert_same(frame(c, pose), before)
    now, built = c.tree_cost()
    assert built > 0 and now > 0
    c.close()


# ---- 2. open the doors ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ["oru4_test", "oru4_legacy"])
def test_open_doors_equal_a_fresh_build_and_the_oracle(native_lib, oracle, table):
    s, mats, objmat, cfg, beams, pose = oru4_setup(table)
    c = make_ctx(native_lib, s, mats, objmat, cfg, beams)
    closed = frame(c, pose)
    P = doors_open(s)
    c.set_object_poses(P)
    got = frame(c, pose)
    soup = posed_soup(s, P)
    assert_same(got, fresh_frame(native_lib, soup, mats, objmat, cfg, beams, pose))
    assert not np.array_equal(got[0], closed[0])                # the doors did move in the image
    oracle_parity(oracle, soup, mats, objmat, cfg, beams, pose, got)
    c.close()


# ---- 3. nearest hit vs brute force ------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", ["host", "gpu"])
def test_trace_after_refits_is_bit_exact_vs_brute_force(native_lib, oracle, builder):
    rs = np.random.RandomState(1)
    n = 6000
    cen = rs.uniform(-30, 30, (n, 1, 3))
    v = (cen + rs.normal(0, 2.0, (n, 3, 3))).astype(np.float32).reshape(-1, 3)
    f = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    obj = np.zeros(n, np.uint32)
    obj[n // 2:] = 1 + (np.arange(n - n // 2) % 4)               # half the triangles in four moving objects
    s = {"verts": v, "faces": f, "face_object_id": obj}
    c = native_lib.Context(0)
    c.set_mesh(v, f, obj, builder=builder)
    info0 = c.bvh_info()
    o = rs.uniform(-35, 35, (20000, 3)).astype(np.float32)
    d = rs.normal(0, 1, (20000, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    d[:50, 1:] = 0.0
    d[:50, 0] = 1.0
    for step in range(2):
        P = identity_poses(5)
        for k in range(1, 5):
            ax = rs.normal(0, 1, 3); ax /= np.linalg.norm(ax)
            ang = rs.uniform(0.5, 3.0)
            P[k, :3] = ax * np.sin(ang / 2); P[k, 3] = np.cos(ang / 2)
            P[k, 4:] = rs.uniform(-25, 25, 3)
        c.set_object_poses(P)
        soup = posed_soup(s, P)
        t, face = c.debug_trace(o, d)
        brute = oracle.Scene(soup["verts"], soup["faces"], None, use_bvh=0)
        hits = 0
        for i in range(0, 20000, 7):
            r = brute.intersect(o[i], d[i])
            if r is None:
                assert t[i] < 0, (step, i)
            else:
                hits += 1
                assert t[i] == np.float32(r[0]) and face[i] == r[1], (step, i)
        assert hits > 500
        assert c.bvh_info() == info0
    c.close()


# ---- 4. deforming mesh + posed building -------------------------------------------------------------------------------
def test_deformed_heightfield_with_a_posed_building_equals_a_fresh_build(native_lib):
    s = scenes.heightfield_room(40, extent=80.0, n_buildings=6, keep_clear=(1.0, 1.5, 6.0))
    mats = materials_for(s)
    cfg = params.kaist_preset(n_reflections=3, ambient_noise=0)
    beams = golden_beams(100)
    pose = scenes.yaw_pose(1.0, 1.5, float(scenes.ground_height(1.0, 1.5)) + 2.0, 0.3)
    c = make_ctx(native_lib, s, mats, s["object_materials"], cfg, beams)
    v2 = s["verts"].copy()
    n_terrain = 41 * 41
    v2[:n_terrain, 2] += (1.5 * np.sin(0.2 * v2[:n_terrain, 0]) * np.cos(0.15 * v2[:n_terrain, 1])).astype(np.float32)
    c.update_vertices(v2)
    P = identity_poses(2)
    P[1] = about((0.0, 0.0, 0.0), 0.4, (2.0, -3.0, 0.5))
    c.set_object_poses(P)
    got = frame(c, pose)
    soup = posed_soup(s, P, verts=v2)
    assert_same(got, fresh_frame(native_lib, soup, mats, s["object_materials"], cfg, beams, pose))
    c.close()


# ---- 5. round trip, tree cost, rebuild --------------------------------------------------------------------------------
def test_round_trip_restores_images_and_cost_and_rebuild_matches(native_lib):
    s, mats, objmat, cfg, beams, pose = oru4_setup()
    c = make_ctx(native_lib, s, mats, objmat, cfg, beams)
    info0 = c.bvh_info()
    c.set_object_poses(identity_poses(18))
    home = frame(c, pose)
    cost_home, built = c.tree_cost()
    # doors, lockers and the bin carried to the other end of the building (inside its shell: the extent stays, and
    # every ancestor of a moved leaf now spans both ends)
    far = identity_poses(18)
    for oid in (3, 4, 6, 7, 8, 12, 14, 16):
        cx = s["verts"][np.unique(s["faces"][s["face_object_id"] == oid])][:, 0].mean()
        far[oid] = about((0, 0, 0), 0.0, (-np.sign(cx) * 12.0, 0.0, 0.0))
    c.set_object_poses(far)
    cost_far, built2 = c.tree_cost()
    assert built2 == built and cost_far > cost_home, (cost_far, cost_home)
    assert c.bvh_info() == info0
    c.set_object_poses(identity_poses(18))
    assert_same(frame(c, pose), home)
    assert c.tree_cost() == (cost_home, built)
    # a rebuild in the far scene: a fresh tree (cost ratio 1), the same images as a fresh context of the soup
    c.set_object_poses(far)
    moved = frame(c, pose)
    for builder in ("host", "gpu"):
        c.rebuild_tree(builder)
        now, at = c.tree_cost()
        assert abs(now / at - 1.0) < 1e-12
        assert_same(frame(c, pose), moved)
    soup = posed_soup(s, far)
    assert_same(moved, fresh_frame(native_lib, soup, mats, objmat, cfg, beams, pose))
    # rest geometry and poses survived the rebuild: back home renders home
    c.set_object_poses(identity_poses(18))
    assert_same(frame(c, pose), home)
    c.close()


# ---- 6. order and launch graphs ---------------------------------------------------------------------------------------
def test_batches_before_a_refit_see_the_old_scene(native_lib):
    s, mats, objmat, cfg, beams, pose = oru4_setup()
    c = make_ctx(native_lib, s, mats, objmat, cfg, beams)
    P = doors_open(s)
    old = frame(c, pose)[0]
    h1 = native_lib.HostImages((4, cfg.n_cells, 400))
    h2 = native_lib.HostImages((4, cfg.n_cells, 400))
    c.simulate_batch_host_async([pose] * 4, h1.ptr)
    c.set_object_poses(P)
    c.simulate_batch_host_async([pose] * 4, h2.ptr)
    c.wait_host()
    new = frame(c, pose)[0]
    assert not np.array_equal(old, new)
    for k in range(4):
        assert np.array_equal(h1.array[k], old) and np.array_equal(h2.array[k], new), k
    h1.close(); h2.close()
    c.close()


def test_refit_keeps_launch_graphs_unless_the_extent_grows(native_lib, monkeypatch):
    import torch
    # one lane, trace rows at the doubling bound: the shape key of a chain cannot change from batch to batch, so every
    # capture after the first is a graph_gen change
    monkeypatch.setenv("RR_LANES", "1")
    monkeypatch.setenv("RR_TIGHT_GRID", "0")
    s, mats, objmat, cfg, beams, pose = oru4_setup()
    c = make_ctx(native_lib, s, mats, objmat, cfg, beams)
    st = torch.cuda.current_stream().cuda_stream
    out = torch.zeros((4, cfg.n_cells, 400), dtype=torch.uint8, device="cuda:0")

    def batch():
        for _ in range(4):
            c.simulate_batch_device([pose] * 4, out.data_ptr(), st)
        c.synchronize(st)
        return out.cpu().numpy().copy()

    batch()
    cap0, rep0 = c.graph_stats()
    assert cap0 >= 1
    P = doors_open(s, 0.5)                                      # inside the building shell: the extent stays
    c.set_object_poses(P)
    got = batch()
    cap1, rep1 = c.graph_stats()
    assert cap1 == cap0 and rep1 > rep0, (cap0, rep0, cap1, rep1)
    want = fresh_frame(native_lib, posed_soup(s, P), mats, objmat, cfg, beams, pose)[0]
    assert all(np.array_equal(got[k], want) for k in range(4))
    # the trash bin thrown far outside: the extent grows, hit_pad changes, the chain is captured again
    P[16] = about((0, 0, 0), 0.0, (0.0, 0.0, 80.0))
    c.set_object_poses(P)
    got = batch()
    cap2, _ = c.graph_stats()
    assert cap2 > cap1
    want = fresh_frame(native_lib, posed_soup(s, P), mats, objmat, cfg, beams, pose)[0]
    assert all(np.array_equal(got[k], want) for k in range(4))
    c.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_scene_untouched(native_lib):
    s, mats, objmat, cfg, beams, pose = oru4_setup()
    c = make_ctx(native_lib, s, mats, objmat, cfg, beams)
    c.set_object_poses(doors_open(s, 0.3))
    before = frame(c, pose)
    cost = c.tree_cost()
    nan_v = s["verts"].copy(); nan_v[5, 1] = np.nan
    inf_v = s["verts"].copy(); inf_v[0, 0] = np.inf
    nan_p = doors_open(s); nan_p[3, 5] = np.nan
    inf_p = doors_open(s); inf_p[12, 4] = -np.inf
    huge = doors_open(s); huge[12, :4] = 1e20                    # finite pose, posed corners overflow
    calls = [lambda: c.update_vertices(s["verts"][:-1]), lambda: c.update_vertices(np.concatenate([s["verts"], s["verts"][:1]])),
             lambda: c.set_object_poses(identity_poses(17)), lambda: c.set_object_poses(identity_poses(19)),
             lambda: c.update_vertices(nan_v), lambda: c.update_vertices(inf_v),
             lambda: c.set_object_poses(nan_p), lambda: c.set_object_poses(inf_p), lambda: c.set_object_poses(huge),
             lambda: c.rebuild_tree(7)]
    for k, call in enumerate(calls):
        with pytest.raises((native_lib.RRError, ValueError)):
            call()
        assert_same(frame(c, pose), before)
        assert c.tree_cost() == cost, k
    empty = native_lib.Context(0)
    for call in (lambda: empty.set_object_poses(identity_poses(1)), lambda: empty.update_vertices(s["verts"]),
                 lambda: empty.rebuild_tree("host"), lambda: empty.tree_cost()):
        with pytest.raises(native_lib.RRError, match="rr_set_mesh"):
            call()
    empty.close()
    c.close()


# ---- 8. copies and rr_multi -------------------------------------------------------------------------------------------
def test_copied_context_is_posed_independently_and_multi_matches(native_lib):
    s, mats, objmat, cfg, beams, pose = oru4_setup()
    a = make_ctx(native_lib, s, mats, objmat, cfg, beams)
    a0 = frame(a, pose)
    b = native_lib.Context(0)
    b.copy_mesh(a)
    b.set_materials(mats, objmat, 0); b.set_config(cfg); b.set_beam_samples(beams)
    P = doors_open(s)
    b.set_object_poses(P)
    want = fresh_frame(native_lib, posed_soup(s, P), mats, objmat, cfg, beams, pose)
    assert_same(frame(b, pose), want)
    assert_same(frame(a, pose), a0)                              # the source did not move
    a.set_object_poses(doors_open(s, -0.5))
    assert_same(frame(b, pose), want)                            # nor does the copy when the source moves
    m = native_lib.MultiContext([0])
    m.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    m.set_materials(mats, objmat, 0); m.set_config(cfg); m.set_beam_samples(beams)
    m.set_object_poses(P)
    assert np.array_equal(m.simulate_batch([pose, pose])[1], want[0])
    m.rebuild_tree("gpu")
    assert np.array_equal(m.simulate(pose), want[0])
    m.update_vertices(s["verts"])
    assert np.array_equal(m.simulate(pose), want[0])
    m.close(); a.close(); b.close()


# ---- 9. scale ---------------------------------------------------------------------------------------------------------
def test_ten_million_triangles_with_moving_vehicles(native_lib, oracle):
    s = scenes.add_vehicles(scenes.config_scene(4), 64)
    mats = materials_for(s)
    cfg = params.kaist_preset(n_reflections=4, ambient_noise=0)
    beams = golden_beams(200)
    pose = scenes.default_pose("heightfield")
    c = make_ctx(native_lib, s, mats, s["object_materials"], cfg, beams, builder="gpu")
    n_obj = int(s["face_object_id"].max()) + 1
    P = identity_poses(n_obj)
    rs = np.random.RandomState(3)
    for oid, cen in zip(s["vehicle_objects"], s["vehicle_centers"]):
        P[oid] = about(cen, rs.uniform(-0.5, 0.5), (rs.uniform(-6, 6), rs.uniform(-6, 6), 0.0))
    c.set_object_poses(P)
    full, _, st = c.simulate(pose)
    # the properties of tests/test_gpu_fullsize.py
    assert st["overflow"] == 0 and st["hits"] > 0.99 * st["wave_passes"] and st["signals"] <= st["hits"]
    assert np.all(full.max(axis=0) == 79) and not full[0].any()
    again, _, st2 = c.simulate(pose)
    assert np.array_equal(full, again) and st2 == st
    # azimuth windows against the oracle on the posed soup
    soup = posed_soup(s, P)
    sc = oracle.Scene(soup["verts"], soup["faces"], soup["face_object_id"], use_bvh=1)
    for az in ((0, 6), (150, 156), (300, 306)):
        g8, gf, gst = c.simulate(pose, az[0], az[1], want_f32=True)
        o8, of, ost = oracle.simulate(sc, mats_tuple(mats), s["object_materials"], cfg, beams, pose, az_begin=az[0], az_end=az[1])
        assert gst["wave_passes"] == ost["wave_passes"] and gst["hits"] == ost["hits"] and gst["signals"] == ost["signals"], az
        d = image_diff(gf, of, g8, o8)
        assert d["mean_dev"] <= MEAN_DEV_TOL and d["u8_max"] <= 1 and d["u8_mismatch_frac"] <= U8_MISMATCH_TOL, (az, d)
    c.close()
