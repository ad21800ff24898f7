"""The host forms' shared staging pool (csrc/rr_stage.h).  Every host form makes its round trip through anonymous slots that other forms
have used before it, so three things can go wrong that named buffers ruled out: bytes left over from another form's call reach the
caller, a slot moves under a pointer handed out earlier, a slot is too small after a small call between two large ones.  Each test runs
a fixed, interleaved sequence of host forms on ONE context -- large, small, larger still -- and holds every call to the same call on a
FRESH context that has made no other: every output byte for byte (both sides run the same kernels on the same bytes: no tolerance),
caller slots beyond a frame's count still at the guard value they were given.

rr_detect's point block is a direct output: the whole [n_frames][max_points] block comes home, as it always has, and the slots beyond a
frame's count hold whatever the device buffer held.  They are compared up to the count; the held row outputs (rr_compensate_points,
rr_register_points' correspondences, the side chains' rows) are compared whole, guard included."""
import numpy as np
import pytest

import field_ref as F
from common import golden_beams
from radarays_ros_amd import native, params, scenes

pytestmark = pytest.mark.gpu

N_CELLS, N_ANGLES = 64, 16
GUARD = 0xA5


def plain_ctx():
    c = native.Context(0)
    c.set_config(params.kaist_preset(n_cells=N_CELLS), N_ANGLES)
    return c


def mesh_ctx():
    s = scenes.box12()
    c = native.Context(0)
    c.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    c.set_materials(params.kaist_materials(), s["object_materials"], 0)
    c.set_config(params.kaist_preset(n_cells=N_CELLS, n_reflections=2, ambient_noise=0), N_ANGLES)
    c.set_beam_samples(golden_beams(100))
    return c


def flat(out):
    """the outputs of a call as a list of (name, bytes)"""
    if not isinstance(out, (tuple, list)):
        out = (out,)
    res = []
    for k, a in enumerate(out):
        if isinstance(a, (tuple, list)):
            res += [("%d.%d" % (k, j), np.ascontiguousarray(b).view(np.uint8).reshape(-1)) for j, b in enumerate(a)]
        elif a is not None:
            res.append((str(k), np.ascontiguousarray(a).view(np.uint8).reshape(-1)))
    return res


def same(name, size, got, want):
    got, want = flat(got), flat(want)
    assert [k for k, _ in got] == [k for k, _ in want], (name, size)
    for (k, a), (_, b) in zip(got, want):
        assert a.size == b.size, (name, size, k)
        diff = np.nonzero(a != b)[0]
        assert diff.size == 0, "%s at %s: output %s differs from a fresh context's first at byte offset %d" % (name, size, k, int(diff[0]))


def run_against_fresh(make_ctx, calls):
    """calls: [(name, size, fn(ctx) -> outputs)]: all of them in turn on one context, each against a context of its own"""
    shared = make_ctx()
    for name, size, fn in calls:
        got = fn(shared)
        fresh = make_ctx()
        want = fn(fresh)
        fresh.close()
        same(name, size, got, want)
    shared.close()


# ---- the inputs: seeded, made once, on the host ---------------------------------------------------------------------------------
def images(rs, n):
    x = (rs.rand(n, N_CELLS, N_ANGLES) ** 6 * 255).astype(np.uint8)      # a few strong cells per column: detections, but not everywhere
    return x


def clouds(n, seed):
    """n frames of detections (offsets [n][N_ANGLES + 1], points [n][total_max]) from a context of their own"""
    rs = np.random.RandomState(seed)
    c = plain_ctx()
    pts, offs = c.detect(images(rs, n), method=1, k=3)
    c.close()
    return pts, offs


def raw_points(pts, mp):
    buf = np.zeros((len(pts), max(mp, 1)), native.POINT_DTYPE)
    for f, p in enumerate(pts):
        buf[f, :min(len(p), mp)] = p[:mp]
    return buf


def detect_raw(ctx, imgs, mp):
    n = len(imgs)
    cfg = native.detect_config(None, n_cells=N_CELLS, method=1, k=3)
    offs = np.full((n, N_ANGLES + 1), 0xA5A5A5A5, np.uint32)
    pts = np.zeros((n, max(mp, 1)), native.POINT_DTYPE)
    ctx._ck(ctx._L.rr_detect(ctx._h, imgs.ctypes.data, n, native.C.byref(cfg), pts.ctypes.data if mp else None, mp, offs.ctypes.data))
    return offs, [pts[f, :min(int(offs[f, -1]), mp)].copy() for f in range(n)]      # (the block beyond a frame's count is unspecified)


def compensate_raw(ctx, pts, offs, table, mp):
    n = len(pts)
    src = raw_points(pts, mp)
    out = np.full((n, max(mp, 1) * native.POINT_DTYPE.itemsize), GUARD, np.uint8).view(native.POINT_DTYPE)
    ctx._ck(ctx._L.rr_compensate_points(ctx._h, src.ctypes.data if mp else None, offs.ctypes.data, n, mp, table.ctypes.data, out.ctypes.data if mp else None))
    raw = out.view(np.uint8).reshape(n, -1)
    for f in range(n):
        assert np.all(raw[f, min(int(offs[f, -1]), mp) * native.POINT_DTYPE.itemsize:] == GUARD), ("rr_compensate_points wrote past a frame's count", f, mp)
    return out


def register_raw(ctx, pts, offs, tgt, mp):
    n = len(pts)
    src = raw_points(pts, mp)
    recs = np.zeros(n, native.ICP_DTYPE)
    corr = np.full((n, max(mp, 1)), 0xA5A5A5A5, np.uint32)
    ctx._ck(ctx._L.rr_register_points(ctx._h, src.ctypes.data if mp else None, offs.ctypes.data, n, mp, tgt.ctypes.data, len(tgt), len(tgt), None,
                                      2.0, 3, recs.ctypes.data, corr.ctypes.data))
    for f in range(n):
        assert np.all(corr[f, min(int(offs[f, -1]), mp):] == 0xA5A5A5A5), ("rr_register_points wrote past a frame's count", f, mp)
    return recs, corr


def rasterize_raw(ctx, pts, offs, grid, mp):
    n = len(pts)
    src = raw_points(pts, mp)
    g = native._field_cfg(grid)
    occ = np.zeros((g.height, g.width), np.uint8)
    occ[0, 0] = 7                                      # the call accumulates
    ctx._ck(ctx._L.rr_rasterize_points(ctx._h, src.ctypes.data if mp else None, offs.ctypes.data, n, mp, None, native.C.byref(g), occ.ctypes.data))
    return occ


def sweep_inputs(rs, n):
    az = np.zeros((n, N_ANGLES, 7), np.float32)
    az[..., 3] = 1.0
    az[..., 4:] = rs.randn(n, N_ANGLES, 3) * 0.2
    ref = az[:, 0].copy()
    return az, ref, (rs.randn(n, 3) * 0.5).astype(np.float32)


def mesh_free_calls():
    calls = []
    rounds = [(5, 8, (16, 8)), (1, 33, (40, 24)), (9, 33, (40, 24))]          # frames or images; Cartesian width; field grid
    for r, (n, width, (gw, gh)) in enumerate(rounds):
        rs = np.random.RandomState(100 + r)
        size = "n=%d width=%d grid=%dx%d" % (n, width, gw, gh)
        imgs, ref = images(rs, n), images(rs, 1)[0]
        pts, offs = clouds(n, 200 + r)
        tgt = np.concatenate(pts)[:40].copy()
        total = int(offs[:, -1].max())
        az, pref, vel = sweep_inputs(rs, n)
        grid = F.grid_cfg(gw, gh, 5)
        planes = rs.randint(0, 4, (n, N_CELLS, N_ANGLES)).astype(np.uint32)
        planes[rs.rand(*planes.shape) < 0.7] = native.LABEL_NONE
        cart = rs.randint(0, 256, (n, width + 16, width + 16)).astype(np.uint8)
        db = rs.randint(0, 256, (70, 4, 8)).astype(np.uint8)
        occ = (rs.rand(gh, gw) < 0.1).astype(np.uint8)
        states = np.tile(np.float32([1, 0, 0, 0]), (n * 7, 1)) + (rs.randn(n * 7, 4) * 0.05).astype(np.float32)
        holder = {}

        def table(c, az=az, pref=pref, vel=vel, holder=holder):
            holder["table"] = c.sweep_table(az, pref, vel, gain=0.01)
            return holder["table"]

        calls += [
            ("rr_compare_images", size, lambda c, imgs=imgs, ref=ref: c.compare_images(imgs, ref, want_hist=True)),
            ("rr_detect (count only)", size, lambda c, imgs=imgs: detect_raw(c, imgs, 0)),
            ("rr_align_images", size, lambda c, imgs=imgs, ref=ref: c.align_images(imgs, ref, want_curve=True)),
            ("rr_sweep_table", size, table),
        ]
        for mp in (total + 1, 0, max(total - 1, 1)):
            tag = "%s max_points=%d" % (size, mp)
            calls += [
                ("rr_detect", tag, lambda c, imgs=imgs, mp=mp: detect_raw(c, imgs, mp)),
                ("rr_compensate_points", tag, lambda c, pts=pts, offs=offs, mp=mp, holder=holder: compensate_raw(c, pts, offs, holder["table"], mp)),
                ("rr_rasterize_points", tag, lambda c, pts=pts, offs=offs, grid=grid, mp=mp: rasterize_raw(c, pts, offs, grid, mp)),
                ("rr_register_points", tag, lambda c, pts=pts, offs=offs, tgt=tgt, mp=mp: register_raw(c, pts, offs, tgt, mp)),
            ]
        calls += [
            ("rr_polar_to_cartesian", size, lambda c, imgs=imgs, width=width: c.polar_to_cartesian(imgs, width, 0.9)),
            ("rr_shift_images", size, lambda c, cart=cart: c.shift_images(cart, cart[0], 3, want_surfaces=True)),
            ("rr_polar_to_cartesian_sweep", size, lambda c, imgs=imgs, width=width, holder=holder: c.polar_to_cartesian_sweep(imgs, holder["table"], width, 0.9)),
            ("rr_describe_images", size, lambda c, imgs=imgs: c.describe_images(imgs, (4, 8))),
            ("rr_distance_field", size, lambda c, occ=occ, grid=grid: c.distance_field(occ, grid)),
            ("rr_match_descriptors", size, lambda c, db=db: c.match_descriptors(db[:3], db, 4, want_full=True)),
            ("rr_score_poses", size, lambda c, p=pts[0], states=states, occ=occ, grid=grid: c.score_poses(p, states, F.distance_field(occ, grid), grid)),
            ("rr_annotate_labels", size, lambda c, planes=planes, imgs=imgs: c.annotate_labels(planes, imgs, n_objects=4)),
            ("rr_polar_to_cartesian_labels", size, lambda c, planes=planes, width=width: c.polar_to_cartesian_labels(planes, width, 0.9)),
        ]
    return calls


def test_mesh_free_host_forms_share_one_pool():
    calls = mesh_free_calls()
    # rr_sweep_table's result feeds later calls: its own comparison runs first, and every context computes the same table
    run_against_fresh(plain_ctx, calls)


def test_simulating_host_forms_share_one_pool():
    pose = np.float32(scenes.default_pose("box12"))
    rs = np.random.RandomState(7)
    ref = images(rs, 1)[0]
    mats = params.kaist_materials()
    n_mat = len(mats)
    calls = []
    for n in (2, 5, 1):
        poses = np.tile(pose, (n, 1))
        poses[:, 4] += np.arange(n, dtype=np.float32) * 0.25
        sets = [{"materials": None, "beam_dirs": None, "n_reflections": 1 + k % 2} for k in range(n)]
        imgs = images(rs, 2 * n)
        size = "n=%d" % n
        calls += [
            ("rr_simulate_batch_align", size, lambda c, poses=poses: c.simulate_batch_align(poses, ref, want_images=True, want_curve=True)),
            ("rr_polar_to_cartesian", size, lambda c, imgs=imgs: c.polar_to_cartesian(imgs, 33, 0.9)),
            ("rr_simulate_batch_shift", size, lambda c, poses=poses: c.simulate_batch_shift(poses, ref, 24, 0.9, 3, want_images=True, want_xcorr=True)),
            ("rr_simulate_batch_describe", size, lambda c, poses=poses: c.simulate_batch_describe(poses, (4, 8))),
            ("rr_compare_images", size, lambda c, imgs=imgs: c.compare_images(imgs, ref, want_hist=True)),
            ("rr_simulate_batch_annotations", size, lambda c, poses=poses: c.simulate_batch_annotations(poses, want_images=True)),
            ("rr_simulate_param_sets", size, lambda c, sets=sets: c.simulate_param_sets(pose, sets, n_mat, ref_u8=ref)),
            ("rr_simulate_param_sets_metrics", size, lambda c, sets=sets: c.simulate_param_sets(pose, sets, n_mat, ref_u8=ref, metrics=native.METRIC_ALL)),
        ]
    run_against_fresh(mesh_ctx, calls)


def test_side_chain_host_forms_share_the_lane_pool():
    pose = np.float32(scenes.default_pose("box12"))
    vel = np.float32([1.5, -0.5, 0.0])
    calls = []
    for r, (labels, faces, stride, f32, vel_img) in enumerate([(True, False, None, True, False), (False, True, 2, False, True)]):
        size = "round %d" % r
        calls += [
            ("rr_simulate_provenance", size, lambda c, labels=labels, faces=faces, stride=stride: c.simulate_provenance(pose, stride, labels, faces)),
            ("rr_simulate_paths", size, lambda c, stride=stride, r=r: c.simulate_paths(pose, stride if r else 0, map_frame=bool(r))),
            ("rr_simulate_doppler", size, lambda c, stride=stride, f32=f32, vel_img=vel_img: c.simulate_doppler(pose, vel, 0.01, stride, f32, vel_img)),
        ]
    run_against_fresh(mesh_ctx, calls)
