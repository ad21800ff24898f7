"""Doppler on the GPU (rr_set_object_twists, rr_simulate_batch_doppler_device, rr_simulate_doppler): the per-echo range rate and the
shifted cell held to their definition (include/radarays_mi355.h; tests/doppler_ref.py fed with the GPU's own wave records and
provenance stream of the same pose, both pinned to the oracle by earlier tests), the image to the oracle's column step on the shifted
stream, the velocity image to the label rule, and the call to itself under other shapes.  Cases, twists and gains are those of
tests/test_doppler_host.py, which proves their premises on the oracle alone."""
import numpy as np
import pytest

import doppler_ref as D
import labels_ref
import test_doppler_host as DH
import test_paths_host as H
from radarays_ros_amd.native import WAVES_MAP_FRAME, RRError
from test_gpu_dynamic import posed_soup
from test_gpu_labels import plain, provenance
from test_gpu_paths import make_ctx, paths

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
A = H.N_ANGLES
SENT = 0x5A
F = np.float32
ESTRIDE = {"N": 400, "A": 4096, "B": 6144, "B2": 6144}          # echoes per azimuth asked for: twice the wave stride of the paths tests


def doppler(c, poses, gain, sensor_vel=None, stride=400, rows=True, vel_img=True, stream=None, sync=True):
    """one Doppler call on device buffers -> (images, v_r [n][A][stride], cells [n][A][stride], counts [n][A], velocity images); the
    bytes behind the last rows are checked to be untouched"""
    poses = np.asarray(poses, np.float32).reshape(-1, 7)
    n = len(poses)
    d_img = torch.zeros((n, c.cfg.n_cells, A), dtype=torch.uint8, device=DEV)
    d_vel = torch.full((n * A * stride * 4 + 64,), SENT, dtype=torch.uint8, device=DEV) if rows else None
    d_cel = torch.full((n * A * stride * 4 + 64,), SENT, dtype=torch.uint8, device=DEV) if rows else None
    d_cnt = torch.full((n, A), -1, dtype=torch.int32, device=DEV)
    d_vi = torch.zeros((n, c.cfg.n_cells, A), dtype=torch.float32, device=DEV) if vel_img else None
    torch.cuda.synchronize()
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    c.simulate_batch_doppler_device(poses, gain, d_img.data_ptr(), sensor_vel, ptr(d_vel), stride if rows else 0, d_cnt.data_ptr(), ptr(d_cel), ptr(d_vi), stream)
    out = (d_img, d_vel, d_cel, d_cnt, d_vi, n, stride)
    return fetch(c, out) if sync else out


def fetch(c, out):
    d_img, d_vel, d_cel, d_cnt, d_vi, n, stride = out
    c.synchronize()
    vel = cel = None
    if d_vel is not None:
        rv, rc = d_vel.cpu().numpy(), d_cel.cpu().numpy()
        assert (rv[n * A * stride * 4:] == SENT).all() and (rc[n * A * stride * 4:] == SENT).all()
        vel, cel = rv[:n * A * stride * 4].view(np.float32).reshape(n, A, stride), rc[:n * A * stride * 4].view(np.int32).reshape(n, A, stride)
    return d_img.cpu().numpy(), vel, cel, d_cnt.cpu().numpy().view(np.uint32).astype(np.int64), None if d_vi is None else d_vi.cpu().numpy()


def written(rows, cnt):
    return [rows[a, :cnt[a]].tobytes() for a in range(A)]


def same(x, y):
    assert np.array_equal(x[0], y[0]) and np.array_equal(x[3], y[3]) and np.array_equal(x[4], y[4], equal_nan=True)
    for f in range(len(x[3])):
        assert written(x[1][f], x[3][f]) == written(y[1][f], y[3][f]) and written(x[2][f], x[3][f]) == written(y[2][f], y[3][f]), f


@pytest.fixture(scope="module")
def ctxs(native_lib):
    cs = {k: make_ctx(native_lib, k) for k in ("N", "B")}
    cs["B2"] = cs["B"]
    yield cs
    for k in ("N", "B"):
        cs[k].close()


_REF = {}


def prior(c, case, rmp):
    """the prior code's outputs for the case's pose, computed once: map-frame and sensor-frame wave records, the provenance stream"""
    if (case, rmp) not in _REF:
        c.set_config(H.config(case, rmp), A)
        _, wm, cnt, _ = paths(c, [H.pose(case)], H.STRIDE[case], flags=WAVES_MAP_FRAME)
        _, ws, _, _ = paths(c, [H.pose(case)], H.STRIDE[case])
        pimg, _, _, ech, ecnt = provenance(c, [H.pose(case)], labels=False, faces=False, stride=ESTRIDE[case])
        assert ecnt.max() <= ESTRIDE[case] and cnt.max() <= H.STRIDE[case]
        _REF[(case, rmp)] = (wm[0], ws[0], cnt[0], ech[0], ecnt[0].astype(np.int64), pimg[0])
    return _REF[(case, rmp)]


def reference(c, case, rmp, gain, twists=DH.TWISTS, v_s=DH.V_S):
    """doppler_ref on the GPU's own records of every azimuth -> (v_r rows, cell rows) as lists per azimuth"""
    wm, ws, cnt, ech, ecnt, _ = prior(c, case, rmp)
    res = c.cfg.resolution
    out = []
    for a in range(A):
        vr, cell, _ = D.doppler(wm[a, :cnt[a]], ws[a, :cnt[a]], int(ecnt[a]), twists, v_s, gain, res)
        out.append((vr, cell))
    return out


# ---- 1. identity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rmp", [False, True], ids=["path", "multipath"])
def test_identity(ctxs, rmp):
    """gain = 0 (zero and nonzero twists), zero twists with zero sensor_vel, sensor_vel = NULL: the plain batch's bytes, the provenance
    stream's cells, v_r = 0 wherever nothing moves; a batch of eight, every pose at several positions"""
    c = ctxs["N"]
    c.set_config(H.config("N", rmp), A)
    poses = [H.L.POSE3[k % 3] for k in range(8)]
    want = plain(c, poses)
    _, _, _, ech, ecnt = provenance(c, poses, labels=False, faces=False, stride=ESTRIDE["N"])
    zeros = np.zeros((8, 3), F)
    moving = np.tile(DH.V_S, (8, 1))
    settings = [("gain0", None, 0.0, zeros, True), ("gain0_moving", DH.TWISTS, 0.0, moving, False), ("zero_twists", None, DH.GAIN, zeros, True),
                ("null_vel", None, DH.GAIN, None, True)]
    rates = None
    for name, tw, gain, vel, still in settings:
        c.set_object_twists(tw)
        img, vr, cel, cnt, vi = doppler(c, poses, gain, vel, stride=ESTRIDE["N"])
        assert np.array_equal(img, want), name
        assert np.array_equal(cnt, ecnt), name
        for f in range(8):
            for a in range(A):
                n = cnt[f, a]
                assert np.array_equal(cel[f, a, :n], ech[f, a, :n]["cell"]), (name, f, a)
                assert not still or not vr[f, a, :n].any(), (name, f, a)
        if not still:
            rates = vr
            assert any(vr[0, a, :cnt[0, a]].any() for a in range(A))
    c.set_object_twists(DH.TWISTS)          # v_r does not depend on the gain
    _, vr2, _, cnt2, _ = doppler(c, poses, DH.GAIN, moving, stride=ESTRIDE["N"])
    for f in range(8):
        assert written(vr2[f], cnt2[f]) == written(rates[f], cnt2[f])
    c.set_object_twists(None)
    assert not np.array_equal(want[0], want[1])


# ---- 2. definition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,gain", [("N", DH.GAIN), ("N", DH.GAIN_EDGE), ("B2", DH.GAIN_EDGE)], ids=["N-gain", "N-edge", "B2-edge"])
def test_rates_and_cells_equal_the_definition(ctxs, case, gain):
    """the f32 bits of every v_r and every cell', all 400 azimuths, path and multipath echoes alike (no tolerance was needed: the GPU's
    sqrtf and division in normalize are correctly rounded); echoes leave the image over both edges (B2: below range zero)"""
    c = ctxs[case]
    ref = reference(c, case, True, gain)
    _, _, _, ech, ecnt, _ = prior(c, case, True)
    c.set_object_twists(DH.TWISTS)
    img, vr, cel, cnt, _ = doppler(c, [H.pose(case)], gain, [DH.V_S], stride=ESTRIDE[case], vel_img=False)
    c.set_object_twists(None)
    assert np.array_equal(cnt[0], ecnt)
    moved = mp = near = far = 0
    for a in range(A):
        n = cnt[0, a]
        rv, rc = ref[a]
        bad = np.flatnonzero(vr[0, a, :n].view(np.uint32) != rv.view(np.uint32))
        assert bad.size == 0, (a, "v_r", bad[:4], vr[0, a, :n][bad[:4]], rv[bad[:4]])
        bad = np.flatnonzero(cel[0, a, :n] != rc)
        assert bad.size == 0, (a, "cell", bad[:4], cel[0, a, :n][bad[:4]], rc[bad[:4]])
        c0 = ech[a, :n]["cell"].astype(np.int64)
        kind = (ech[a, :n]["info"] >> np.uint32(28)) & np.uint32(1)
        moved += int((rc != c0).sum()); mp += int(((kind == 1) & (rc != c0)).sum())
        near += int((rc == -1).sum()); far += int(((c0 < c.cfg.n_cells) & (rc >= c.cfg.n_cells)).sum())
    assert moved > 0 and mp > 0 and (gain == DH.GAIN or far > 0) and (case != "B2" or near > 0), (moved, mp, near, far)


# ---- 3. image, 4. velocity image ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scroll", [0, 37])
def test_image_and_velocity_image(ctxs, oracle, scroll):
    """d_imgs_u8 and out_f32 against the oracle's column step on the shifted stream (exact, as tests/test_gpu_column.py holds streams
    without ambient noise); the velocity image against the winner column of doppler_ref, NaN exactly where nobody reaches the bin"""
    c = ctxs["N"]
    ref = reference(c, "N", True, DH.GAIN_EDGE)
    _, _, _, ech, ecnt, pimg = prior(c, "N", True)
    cfg = H.L.config(3, True, scroll_image=scroll)
    c.set_config(cfg, A)
    c.set_object_twists(DH.TWISTS)
    img, _, _, cnt, vi = doppler(c, [H.pose("N")], DH.GAIN_EDGE, [DH.V_S], stride=ESTRIDE["N"])
    u8, f32, hv, hc, hcnt, hvi = c.simulate_doppler(H.pose("N"), DH.V_S, DH.GAIN_EDGE, want_f32=True)
    c.set_object_twists(None)
    assert np.array_equal(u8, img[0]) and np.array_equal(hvi, vi[0], equal_nan=True) and np.array_equal(hcnt, cnt[0]) and hv.shape == (A, cnt.max())
    w, mode = labels_ref.weights(cfg, oracle)
    winners = 0
    for a in range(A):
        n = int(ecnt[a])
        rv, rc = ref[a]
        assert np.array_equal(hc[a, :n], rc) and np.array_equal(hv[a, :n].view(np.uint32), rv.view(np.uint32))
        col = (scroll + a) % A
        rf, r8 = oracle.column(cfg, rc.astype(np.int32), ech[a, :n]["strength"], 0.0, col, A)
        assert np.array_equal(f32[:, col], rf, equal_nan=True), (a, np.flatnonzero(f32[:, col] != rf)[:8])
        assert np.array_equal(img[0][:, col], r8), (a, np.flatnonzero(img[0][:, col] != r8)[:8])
        want = D.winner_column(rc, ech[a, :n]["strength"], rv, cfg.n_cells, w, mode)
        assert np.array_equal(vi[0][:, col].view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)]), a
        assert np.array_equal(np.isnan(vi[0][:, col]), np.isnan(want)), a
        winners += int((~np.isnan(want)).sum())
    assert winners > 0 and np.isnan(vi).any() and (scroll == 0 or not np.array_equal(img[0], pimg))
    c.set_config(H.config("N", True), A)


# ---- 5. dynamic scenes --------------------------------------------------------------------------------------------------------------
def test_moved_object_equals_a_fresh_context_of_the_posed_soup(native_lib):
    s = H.scene("N")
    poses = np.float32([[0, 0, 0, 1, 0, 0, 0], [0, 0, np.sin(0.1), np.cos(0.1), 0.2, -0.1, 0.05]])
    c = make_ctx(native_lib, "N")
    c.set_object_twists(DH.TWISTS)
    rest = doppler(c, [H.pose("N")], DH.GAIN, [DH.V_S])
    c.set_object_poses(poses)            # (the twists stay)
    moved = doppler(c, [H.pose("N")], DH.GAIN, [DH.V_S])
    d = make_ctx(native_lib, "N", scene=posed_soup(s, poses))
    d.set_object_twists(DH.TWISTS)
    fresh = doppler(d, [H.pose("N")], DH.GAIN, [DH.V_S])
    same(moved, fresh)
    assert written(moved[1][0], moved[3][0]) != written(rest[1][0], rest[3][0])
    c.close(); d.close()


# ---- 6. shapes ----------------------------------------------------------------------------------------------------------------------
def test_short_rows_keep_true_counts(ctxs):
    c = ctxs["N"]
    c.set_config(H.config("N", True), A)
    c.set_object_twists(DH.TWISTS)
    full = doppler(c, [H.pose("N")], DH.GAIN, [DH.V_S])
    short = 50
    assert short < full[3].min()
    cut = doppler(c, [H.pose("N")], DH.GAIN, [DH.V_S], stride=short)          # (doppler() checks the guard bytes behind the last row)
    assert np.array_equal(cut[0], full[0]) and np.array_equal(cut[3], full[3]) and np.array_equal(cut[4], full[4], equal_nan=True)
    assert cut[1][0].tobytes() == np.ascontiguousarray(full[1][0][:, :short]).tobytes() and cut[2][0].tobytes() == np.ascontiguousarray(full[2][0][:, :short]).tobytes()
    u8, _, hv, hc, hcnt, _ = c.simulate_doppler(H.pose("N"), DH.V_S, DH.GAIN, echo_stride=short)
    assert np.array_equal(u8, full[0][0]) and np.array_equal(hcnt, full[3][0]) and hv.tobytes() == cut[1][0].tobytes() and hc.tobytes() == cut[2][0].tobytes()
    none = doppler(c, [H.pose("N")], DH.GAIN, [DH.V_S], rows=False, vel_img=False)          # counts alone
    assert np.array_equal(none[0], full[0]) and np.array_equal(none[3], full[3])
    c.set_object_twists(None)


def test_two_calls_on_different_lanes(ctxs):
    c = ctxs["N"]
    c.set_config(H.config("N", True), A)
    c.set_object_twists(DH.TWISTS)
    singles = [doppler(c, [H.L.POSE3[k]], DH.GAIN, [DH.V_S]) for k in (0, 1)]
    pending = [doppler(c, [H.L.POSE3[k]], DH.GAIN, [DH.V_S], sync=False) for k in (0, 1)]          # consecutive calls take consecutive lanes
    for k in (0, 1):
        same(fetch(c, pending[k]), singles[k])
    assert written(singles[0][1][0], singles[0][3][0]) != written(singles[1][1][0], singles[1][3][0])
    c.set_object_twists(None)


def test_gpu_tree_builder_gives_the_same_result(ctxs, native_lib):
    c = ctxs["N"]
    c.set_config(H.config("N", True), A)
    c.set_object_twists(DH.TWISTS)
    base = doppler(c, [H.pose("N")], DH.GAIN, [DH.V_S])
    c.set_object_twists(None)
    g = make_ctx(native_lib, "N", builder="gpu")
    g.set_object_twists(DH.TWISTS)
    same(doppler(g, [H.pose("N")], DH.GAIN, [DH.V_S]), base)
    g.close()


def test_no_pass_gives_no_echo(native_lib):
    c = make_ctx(native_lib, "N")
    c.set_config(H.L.config(0, True), A)
    c.set_object_twists(DH.TWISTS)
    img, vr, cel, cnt, vi = doppler(c, [H.pose("N")], DH.GAIN, [DH.V_S], stride=4)
    assert not cnt.any() and not img.any() and np.isnan(vi).all() and (vr.view(np.uint8) == SENT).all() and (cel.view(np.uint8) == SENT).all()
    c.close()


def test_include_motion_uses_each_azimuths_own_origin(native_lib):
    """a table that holds the call's pose for every azimuth is the plain call; under a table of its own the outputs are doppler_ref's
    on the paths records of the same table, whose pass-0 origins (the t_am of the multipath term) differ per azimuth"""
    c = make_ctx(native_lib, "N")
    c.set_object_twists(DH.TWISTS)
    pose = np.asarray(H.pose("N"), np.float32)
    base = doppler(c, [pose], DH.GAIN, [DH.V_S])
    c.set_motion_poses(np.broadcast_to(pose, (A, 7)).copy())
    same(doppler(c, [H.L.POSE3[1]], DH.GAIN, [DH.V_S]), base)          # the call's own pose is not looked at
    table = np.broadcast_to(pose, (A, 7)).copy()
    table[:, 4] += np.linspace(0.0, 0.5, A, dtype=np.float32)
    c.set_motion_poses(table)
    _, wm, cnt, _ = paths(c, [pose], H.STRIDE["N"], flags=WAVES_MAP_FRAME)
    _, ws, _, _ = paths(c, [pose], H.STRIDE["N"])
    img, vr, cel, ecnt, _ = doppler(c, [pose], DH.GAIN, [DH.V_S])
    multipath = 0
    for a in range(A):
        assert np.array_equal(wm[0, a, 0]["o"], table[a, 4:])
        n = int(ecnt[0, a])
        rv, rc, _ = D.doppler(wm[0, a, :cnt[0, a]], ws[0, a, :cnt[0, a]], n, DH.TWISTS, DH.V_S, DH.GAIN, c.cfg.resolution)
        assert np.array_equal(vr[0, a, :n].view(np.uint32), rv.view(np.uint32)) and np.array_equal(cel[0, a, :n], rc), a
        multipath += int((wm[0, a, :cnt[0, a]]["info"] >> np.uint32(31)).sum())
    assert multipath > 0 and written(vr[0], ecnt[0]) != written(base[1][0], base[3][0])
    c.close()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ctxs, native_lib):
    c = ctxs["N"]
    c.set_config(H.config("N", True), A)
    c.set_object_twists(DH.TWISTS)
    before = doppler(c, [H.pose("N")], DH.GAIN, [DH.V_S])
    Lb, h = native_lib.lib(), c._h
    # rr_set_object_twists: wrong count, non-finite value -> the previous twists still act
    bad = DH.TWISTS.copy(); bad[1, 4] = np.inf
    three = np.zeros((3, 6), F)
    assert Lb.rr_set_object_twists(h, three.ctypes.data, 3) == -3 and "expected 2 twists" in Lb.rr_last_error(h).decode()
    assert Lb.rr_set_object_twists(h, bad.ctypes.data, 2) == -3 and "non-finite" in Lb.rr_last_error(h).decode()
    assert Lb.rr_set_object_twists(h, None, 2) == -3
    with pytest.raises(RRError):
        c.set_object_twists(np.zeros((1, 6), F))
    with pytest.raises(ValueError):
        c.set_object_twists(np.zeros((2, 5), F))
    same(doppler(c, [H.pose("N")], DH.GAIN, [DH.V_S]), before)
    pose = np.asarray(H.pose("N"), np.float32)
    vs, nanv = DH.V_S.copy(), np.float32([0, np.nan, 0])
    buf = torch.full((8192,), SENT, dtype=torch.uint8, device=DEV)
    img, vel, cel, cn, vi = (buf.data_ptr() + 1024 * k for k in range(5))
    P = pose.ctypes.data
    calls = [((None, 1, vs.ctypes.data, 0.1, img, vel, 1, cn, cel, vi, None), "null poses/output"), ((P, 1, vs.ctypes.data, 0.1, None, vel, 1, cn, cel, vi, None), "null poses/output"),
             ((P, 1, vs.ctypes.data, 0.1, img, vel, 1, None, None, vi, None), "needs a count buffer"), ((P, 1, vs.ctypes.data, 0.1, img, None, 1, None, cel, vi, None), "needs a count buffer"),
             ((P, 1, vs.ctypes.data, 0.1, img, vel, 0, cn, cel, vi, None), "echo_stride must be positive"),
             ((P, 0, vs.ctypes.data, 0.1, img, vel, 1, cn, cel, vi, None), "n_frames must be 1..64"), ((P, 65, vs.ctypes.data, 0.1, img, vel, 1, cn, cel, vi, None), "n_frames must be 1..64"),
             ((P, 1, vs.ctypes.data, float("nan"), img, vel, 1, cn, cel, vi, None), "non-finite gain"), ((P, 1, vs.ctypes.data, float("inf"), img, vel, 1, cn, cel, vi, None), "non-finite gain"),
             ((P, 1, nanv.ctypes.data, 0.1, img, vel, 1, cn, cel, vi, None), "non-finite sensor velocity")]
    for args, msg in calls:
        assert Lb.rr_simulate_batch_doppler_device(h, *args) == -3 and msg in Lb.rr_last_error(h).decode(), (args, Lb.rr_last_error(h))
    h8, hv, hc = np.full(c.cfg.n_cells * A, SENT, np.uint8), np.full(64, SENT, np.uint8), np.full(4 * A, SENT, np.uint8)
    assert Lb.rr_simulate_doppler(h, P, vs.ctypes.data, 0.1, h8.ctypes.data, None, hv.ctypes.data, 1, None, None, None) == -3 and "needs a count buffer" in Lb.rr_last_error(h).decode()
    assert Lb.rr_simulate_doppler(h, P, vs.ctypes.data, 0.1, h8.ctypes.data, None, hv.ctypes.data, 0, hc.ctypes.data, None, None) == -3
    assert Lb.rr_simulate_doppler(h, P, nanv.ctypes.data, 0.1, h8.ctypes.data, None, None, 0, hc.ctypes.data, None, None) == -3
    assert Lb.rr_simulate_doppler(h, P, vs.ctypes.data, float("nan"), h8.ctypes.data, None, None, 0, hc.ctypes.data, None, None) == -3
    assert Lb.rr_simulate_doppler(h, None, vs.ctypes.data, 0.1, h8.ctypes.data, None, None, 0, hc.ctypes.data, None, None) == -3
    bare = native_lib.Context(0)
    assert Lb.rr_set_object_twists(bare._h, DH.TWISTS.ctypes.data, 2) == -2 and Lb.rr_last_error(bare._h)          # no mesh
    assert Lb.rr_simulate_batch_doppler_device(bare._h, P, 1, None, 0.1, img, vel, 1, cn, cel, vi, None) == -2
    bare.set_config(H.config("N", True), A)
    assert Lb.rr_simulate_batch_doppler_device(bare._h, P, 1, None, 0.1, img, vel, 1, cn, cel, vi, None) == -2          # no mesh
    bare.close()
    c.synchronize()
    assert (buf.cpu().numpy() == SENT).all() and (h8 == SENT).all() and (hv == SENT).all() and (hc == SENT).all()
    same(doppler(c, [H.pose("N")], DH.GAIN, [DH.V_S]), before)
    c.set_object_twists(None)


def test_velocity_image_at_the_label_limit(native_lib):
    """RR_LABEL_MAX_CELLS applies to the velocity image alone, and it is the most rr_set_config admits: a wider column never gets as
    far as a Doppler call, and at the limit itself (64 KB of keys in LDS) the velocity image is made"""
    import dataclasses
    c = make_ctx(native_lib, "N")
    with pytest.raises(RRError):
        c.set_config(dataclasses.replace(H.config("N", True), n_cells=native_lib.LABEL_MAX_CELLS + 1), A)
    c.set_config(dataclasses.replace(H.config("N", True), n_cells=native_lib.LABEL_MAX_CELLS), A)
    c.set_object_twists(DH.TWISTS)
    img, vr, cel, cnt, vi = doppler(c, [H.pose("N")], DH.GAIN, [DH.V_S])
    assert cnt.min() > 0 and img.any() and (~np.isnan(vi)).any() and np.isnan(vi).any()
    c.close()


# ---- 8. the plain path is untouched -------------------------------------------------------------------------------------------------
def test_plain_batches_keep_their_graph_and_their_bytes(native_lib, monkeypatch):
    monkeypatch.setenv("RR_LANES", "1")          # one frame lane: every batch meets the same buffers (and the same graph)
    c = make_ctx(native_lib, "N")
    poses = H.L.POSE3
    want = plain(c, poses)
    for _ in range(2):
        assert np.array_equal(plain(c, poses), want)
    cap, rep = c.graph_stats()
    assert cap >= 1 and rep >= 1, (cap, rep)
    c.set_object_twists(DH.TWISTS)
    assert c.graph_stats() == (cap, rep)
    img, vr, cel, cnt, vi = doppler(c, poses, DH.GAIN, np.tile(DH.V_S, (3, 1)))
    assert not np.array_equal(img, want) and cnt.min() > 0 and c.graph_stats() == (cap, rep)
    assert np.array_equal(plain(c, poses), want) and c.graph_stats() == (cap, rep + 1)
    st = c.stats()
    assert st["wave_passes"] > 0
    c.close()
