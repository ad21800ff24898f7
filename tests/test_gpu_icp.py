"""Scan matching on the GPU (rr_icp.hip) against the numpy restatement of its definition (tests/icp_ref.py), bit for bit: the state as
raw f64 bits, sse, n_matched, flags and every correspondence, at the edges of the source and target tiling, with truncated, NaN, lattice,
gated-out and aliased clouds; the same bytes whatever the order of arrival and on two streams at once; and a closed loop through the
simulator in which the relative pose of two scans of a room comes back within the bound test_icp_host.py fixed."""
import math

import numpy as np
import pytest

import icp_ref as R
from common import golden_beams
from radarays_ros_amd import native, params, radar

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
N_ANGLES = 16
GUARD = 0xA5
GATE = 1.5


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    c.set_config(params.kaist_preset(n_cells=64), N_ANGLES)
    return c


@pytest.fixture(scope="module")
def tiles():
    return native.icp_tile_sizes()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)


def target_cloud(rs, count):
    return rs.uniform(-20, 20, (count, 2)).astype(np.float32)


def source_cloud(rs, tgt, count, yaw=0.04, t=(0.3, -0.2), noise=0.05):
    """`count` points of the target (cycled at random), jittered, seen from a frame that the transform (yaw, t) maps into the target's"""
    if count == 0 or len(tgt) == 0:
        return rs.uniform(-20, 20, (count, 2)).astype(np.float32)
    q = tgt[rs.randint(0, len(tgt), count)].astype(np.float64) + rs.normal(0, noise, (count, 2)) - np.asarray(t)
    c, s = math.cos(yaw), math.sin(yaw)
    return np.stack([c * q[:, 0] + s * q[:, 1], -s * q[:, 0] + c * q[:, 1]], -1).astype(np.float32)


def run_device(ctx, clouds, tgt, init=None, gate=GATE, iterations=2, max_points=None, max_tgt=None, want_corr=True, stream=None, alias=False):
    """the device form on guarded buffers -> (records ICP_DTYPE [n], the whole correspondence buffer uint32 [n][max_points] or None).
    clouds / tgt: [m][2] arrays; a cloud longer than max_points keeps its true total in the offsets and loses its tail"""
    n = len(clouds)
    mp = max(1, max(len(c) for c in clouds)) if max_points is None else max_points
    mt = max(1, len(tgt)) if max_tgt is None else max_tgt
    pts = np.zeros((n, mp), native.POINT_DTYPE)
    offs = np.zeros((n, N_ANGLES + 1), np.uint32)
    for f, c in enumerate(clouds):
        pts[f, :min(len(c), mp)] = R.points_of(c[:mp])
        offs[f, 1:] = len(c)
    if alias:                                                        # the target IS frame 0 of the sources, its count frame 0's total
        d_pts, d_offs = dev(pts), dev(offs)
        tgt_ptr, cnt_ptr = d_pts.data_ptr(), d_offs.data_ptr() + 4 * N_ANGLES
    else:
        t = np.zeros(mt, native.POINT_DTYPE)
        t[:min(len(tgt), mt)] = R.points_of(tgt[:mt])
        d_pts, d_offs, d_tgt, d_cnt = dev(pts), dev(offs), dev(t), dev(np.array([len(tgt)], np.uint32))
        tgt_ptr, cnt_ptr = d_tgt.data_ptr(), d_cnt.data_ptr()
    d_init = None if init is None else dev(np.ascontiguousarray(init, np.float64))
    d_rec = torch.full((n * 48 + 48,), GUARD, dtype=torch.uint8, device=DEV)
    d_corr = torch.full((n * mp * 4 + 64,), GUARD, dtype=torch.uint8, device=DEV) if want_corr else None
    torch.cuda.synchronize()
    ctx.register_points_device(d_pts.data_ptr(), d_offs.data_ptr(), n, mp, tgt_ptr, cnt_ptr, mt, d_rec.data_ptr(),
                               None if d_init is None else d_init.data_ptr(), gate, iterations, d_corr.data_ptr() if want_corr else None, stream)
    torch.cuda.synchronize()
    rec = d_rec.cpu().numpy()
    assert np.all(rec[n * 48:] == GUARD)                             # nothing behind the records
    corr = None
    if want_corr:
        raw = d_corr.cpu().numpy()
        assert np.all(raw[n * mp * 4:] == GUARD)                     # ... or behind the correspondences
        corr = raw[:n * mp * 4].view(np.uint32).reshape(n, mp)
    return rec[:n * 48].view(native.ICP_DTYPE).copy(), corr


def same_as_ref(rec, corr, want_rec, want_corr):
    for k in ("c", "s", "tx", "ty"):
        assert np.array_equal(rec[k].view(np.uint64), want_rec[k].view(np.uint64)), (k, rec[k], want_rec[k])
    for k in ("sse", "n_matched", "flags"):
        assert np.array_equal(rec[k], want_rec[k]), (k, rec[k], want_rec[k])
    if corr is not None:
        guard = np.uint32(GUARD * 0x01010101)
        for f, w in enumerate(want_corr):
            assert np.array_equal(corr[f, :len(w)], w), f
            assert np.all(corr[f, len(w):] == guard), f              # nothing past the frame's count


def check(ctx, clouds, tgt, init=None, gate=GATE, iterations=2, max_points=None, max_tgt=None, **kw):
    rec, corr = run_device(ctx, clouds, tgt, init, gate, iterations, max_points, max_tgt, **kw)
    want_rec, _, want_corr = R.register(clouds, tgt, init, gate, iterations, max_points, max_tgt)
    same_as_ref(rec, corr, want_rec, want_corr)
    return rec, corr


# ---- 1. the tiling edges ------------------------------------------------------------------------------------------------
def edge_cases(tiles):
    S, T = tiles
    a, b = [0, 1, 2, 63, 2 * S + 1], [64, 65, S - 1, S, S + 1]
    return [(a, T + 1), (b, 2 * T + 1), (b, 1), (a, T - 1), (b, T), ([S + 1], T + 1)]


_EDGE = {}


def edge_inputs(tiles, case):
    """a case's clouds, made once and shared by the three iteration counts"""
    if case not in _EDGE:
        counts, n_tgt = edge_cases(tiles)[case]
        rs = np.random.RandomState(100 + case)
        tgt = target_cloud(rs, n_tgt)
        clouds = [source_cloud(rs, tgt, m, yaw=0.02 * (f + 1), t=(0.1 * f, -0.2)) for f, m in enumerate(counts)]
        init = native.se2_states(rs.uniform(-0.03, 0.03, len(counts)), rs.uniform(-0.2, 0.2, len(counts)), rs.uniform(-0.2, 0.2, len(counts)))
        init[:, :2] *= 1.7                                           # not normalised: the call does that
        _EDGE[case] = (clouds, tgt, init)
    return _EDGE[case]


@pytest.mark.parametrize("iterations", [0, 1, 8])
@pytest.mark.parametrize("case", range(6))
def test_tiling_edges_match_the_restatement(ctx, tiles, case, iterations):
    clouds, tgt, init = edge_inputs(tiles, case)
    rec, _ = check(ctx, clouds, tgt, init, iterations=iterations)
    if len(tgt) > 1:
        assert rec["n_matched"].max() > 0.5 * max(len(c) for c in clouds)      # the comparison is not of empty sums


def test_null_init_and_null_corr(ctx, tiles):
    clouds, tgt, _ = edge_inputs(tiles, 0)
    rec, _ = check(ctx, clouds, tgt, None, iterations=3)
    rec2, corr2 = check(ctx, clouds, tgt, None, iterations=3, want_corr=False)
    assert corr2 is None and rec.tobytes() == rec2.tobytes()
    ident = native.se2_states(np.zeros(len(clouds)))
    assert run_device(ctx, clouds, tgt, ident, iterations=3)[0].tobytes() == rec.tobytes()


# ---- 2. truncation ------------------------------------------------------------------------------------------------------
def test_truncated_source_and_target(ctx, tiles):
    S, T = tiles
    rs = np.random.RandomState(7)
    tgt = target_cloud(rs, T + 40)
    clouds = [source_cloud(rs, tgt, m) for m in (S + 30, 17, S + 1)]
    rec, _ = check(ctx, clouds, tgt, iterations=2, max_points=S + 1)
    assert list(rec["flags"] & R.TRUNCATED) == [R.TRUNCATED, 0, 0]
    rec, corr = check(ctx, clouds, tgt, iterations=2, max_tgt=T - 3)
    matched = corr[(corr != np.uint32(GUARD * 0x01010101)) & (corr != R.NONE)]
    assert np.all(rec["flags"] & R.TRUNCATED) and len(matched) > S and matched.max() < T - 3


# ---- 3. exact ties ------------------------------------------------------------------------------------------------------
def test_lattice_ties_go_to_the_lower_index(ctx, tiles):
    S, T = tiles
    side = int(math.ceil(math.sqrt(T + 200)))                        # an integer lattice that crosses a target tile's edge
    g = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2).astype(np.float32) - side // 2
    assert len(g) > T
    rs = np.random.RandomState(3)
    pick = g[rs.randint(0, len(g), S + 70)]
    clouds = [pick + np.float32([0.5, 0.5]), pick + np.float32([0.5, 0.0]), pick]     # ties between 4, between 2, none
    rec, corr = check(ctx, clouds, g, iterations=0)
    # the cell centre is equally far from four lattice points: the one with the lowest index is (i, j) itself, before (i, j + 1), (i + 1, j) ...
    want = (pick[:, 0] + side // 2) * side + (pick[:, 1] + side // 2)
    keep = (pick[:, 0] + side // 2 < side - 1) & (pick[:, 1] + side // 2 < side - 1)
    assert np.array_equal(corr[0, :len(pick)][keep], want[keep].astype(np.uint32))
    assert np.array_equal(corr[2, :len(pick)], want.astype(np.uint32)) and rec["sse"][2] == 0
    check(ctx, clouds, g, iterations=2)


# ---- 4. points that are not points ----------------------------------------------------------------------------------------
def test_nan_and_out_of_range_points(ctx, tiles):
    S, T = tiles
    rs = np.random.RandomState(11)
    tgt = target_cloud(rs, T + 9)
    tgt[rs.randint(0, len(tgt), 40)] = np.nan                        # what rr_compensate_points writes for a point without a range
    tgt[5] = (8192.0, 0.0); tgt[T] = (1.0, -9000.0); tgt[T + 1] = (np.inf, 1.0); tgt[7, 1] = np.nan
    clouds = [source_cloud(rs, target_cloud(rs, 300), m) for m in (S + 5, 90)]
    clouds[0][rs.randint(0, S + 5, 50)] = np.nan
    clouds[0][3] = (8192.0, 1.0); clouds[0][4] = (-1e30, 1.0); clouds[0][6] = (np.inf, -np.inf); clouds[1][0, 0] = np.nan
    rec, corr = check(ctx, clouds, tgt, iterations=3, gate=3.0)
    assert rec["n_matched"][0] > 100
    bad = np.nonzero(~(np.abs(tgt).max(axis=1) < 8192))[0]
    assert len(bad) >= 40 and not np.isin(corr[0, :S + 5], bad).any()
    # a target of nothing but such points
    rec, corr = check(ctx, clouds, tgt[bad], iterations=2)
    assert np.all(rec["n_matched"] == 0) and np.all(rec["flags"] == R.DEGENERATE)


def test_a_frame_beyond_the_gate_is_degenerate_and_keeps_its_state(ctx):
    rs = np.random.RandomState(13)
    tgt = target_cloud(rs, 200)
    clouds = [source_cloud(rs, tgt, 150), target_cloud(rs, 150) + np.float32(1000.0), source_cloud(rs, tgt, 1)]
    init = native.se2_states([0.01, 0.3, -0.2], [0.1, 5.0, 0.0], [0.0, -4.0, 0.1])
    rec, corr = check(ctx, clouds, tgt, init, iterations=4)
    assert list(rec["flags"]) == [0, R.DEGENERATE, R.DEGENERATE] and rec["n_matched"][1] == 0 and np.all(corr[1, :150] == R.NONE)
    assert (rec["c"][1], rec["s"][1], rec["tx"][1], rec["ty"][1]) == R.normalise(init[1])[0]


def test_degenerate_initial_states_become_the_identity(ctx):
    rs = np.random.RandomState(14)
    tgt = target_cloud(rs, 50)
    clouds = [source_cloud(rs, tgt, 40, yaw=0.0, t=(0, 0), noise=0.0)] * 3
    init = np.array([[0.0, 0.0, 3.0, 3.0], [np.nan, 1.0, 0.0, 0.0], [2.0, 0.0, 0.0, 0.0]])
    rec, _ = check(ctx, clouds, tgt, init, iterations=0)
    assert list(rec["flags"]) == [R.DEGENERATE, R.DEGENERATE, 0] and np.all(rec["c"] == 1.0) and np.all(rec["n_matched"] == 40)


# ---- 5. aliasing, the host form ---------------------------------------------------------------------------------------------
def test_a_cloud_against_itself(ctx, tiles):
    S, _ = tiles
    rs = np.random.RandomState(17)
    clouds = [target_cloud(rs, S + 3), target_cloud(rs, 40)]
    rec, corr = run_device(ctx, clouds, clouds[0], None, GATE, 2, alias=True)
    want_rec, _, want_corr = R.register(clouds, clouds[0], None, GATE, 2)
    same_as_ref(rec, corr, want_rec, want_corr)
    assert (rec["c"][0], rec["s"][0], rec["tx"][0], rec["ty"][0], rec["sse"][0], rec["n_matched"][0]) == (1.0, 0.0, 0.0, 0.0, 0, S + 3)
    assert np.array_equal(corr[0, :S + 3], np.arange(S + 3))


def test_the_host_form_equals_the_device_form(ctx, tiles):
    clouds, tgt, init = edge_inputs(tiles, 0)
    rec, corr = run_device(ctx, clouds, tgt, init, GATE, 3)
    offs = np.zeros((len(clouds), N_ANGLES + 1), np.uint32)
    offs[:, -1] = [len(c) for c in clouds]
    h_rec, h_corr = ctx.register_points([R.points_of(c) for c in clouds], offs, R.points_of(tgt), init, GATE, 3, want_corr=True)
    assert h_rec.tobytes() == rec.tobytes()
    for f, c in enumerate(clouds):
        assert np.array_equal(h_corr[f], corr[f, :len(c)])
    assert ctx.register_points([R.points_of(c) for c in clouds], offs, R.points_of(tgt), init, GATE, 3).tobytes() == rec.tobytes()
    # what the host form can see and the device form cannot
    bad = init.copy()
    bad[1, :2] = 0.0
    L = ctx._L
    pts = np.zeros((2, 4), native.POINT_DTYPE)
    o = np.zeros((2, N_ANGLES + 1), np.uint32)
    out = np.full(2 * 48, GUARD, np.uint8)
    t = R.points_of(tgt[:4])
    args = lambda i, gate=1.0, it=1, n=2, mp=4: (ctx._h, pts.ctypes.data, o.ctypes.data, n, mp, t.ctypes.data, 4, 4, i, gate, it, out.ctypes.data, None)   # noqa: E731
    assert L.rr_register_points(*args(bad[:2].ctypes.data)) == -3 and b"rr_register_points" in L.rr_last_error(ctx._h)
    for kw in (dict(gate=0.0), dict(gate=float("nan")), dict(gate=float("inf")), dict(it=-1), dict(it=65), dict(n=0), dict(n=65536), dict(mp=65537),
               dict(mp=-1)):
        assert L.rr_register_points(*args(None, **kw)) == -3, kw
    assert np.all(out == GUARD)
    d = torch.full((256,), GUARD, dtype=torch.uint8, device=DEV)
    p = d.data_ptr()
    for a in ((None, p, 2, 4, p, p, 4, None, 1.0, 1, p, None), (p, None, 2, 4, p, p, 4, None, 1.0, 1, p, None), (p, p, 2, 4, None, p, 4, None, 1.0, 1, p, None),
              (p, p, 2, 4, p, None, 4, None, 1.0, 1, p, None), (p, p, 2, 4, p, p, 4, None, 1.0, 1, None, None), (p, p, 2, 4, p, p, 4, p + 4, 1.0, 1, p, None),
              (p, p, 2, 4, p, p, 4, None, 1.0, 1, p + 4, None), (p, p, 2, 4, p, p, 65537, None, 1.0, 1, p, None), (p, p, 2, 4, p, p, 4, None, -1.0, 1, p, None)):
        assert L.rr_register_points_device(ctx._h, *a, None) == -3, a
    bare = native.Context(0)
    assert bare._L.rr_register_points_device(bare._h, p, p, 2, 4, p, p, 4, None, 1.0, 1, p, None, None) == -2
    torch.cuda.synchronize()
    assert bool((d == GUARD).all())


# ---- 6. order independence, two streams ---------------------------------------------------------------------------------
def test_the_same_bytes_twice_and_with_the_frames_permuted(ctx, tiles):
    clouds, tgt, init = edge_inputs(tiles, 1)
    first = run_device(ctx, clouds, tgt, init, GATE, 5)
    again = run_device(ctx, clouds, tgt, init, GATE, 5)
    assert first[0].tobytes() == again[0].tobytes() and np.array_equal(first[1], again[1])
    perm = [3, 0, 4, 2, 1]
    rec, corr = run_device(ctx, [clouds[k] for k in perm], tgt, init[perm], GATE, 5)
    for at, k in enumerate(perm):
        assert rec[at].tobytes() == first[0][k].tobytes() and np.array_equal(corr[at, :len(clouds[k])], first[1][k, :len(clouds[k])])


def loop_context():
    s, cfg = R.loop_scene(), R.loop_cfg()
    c = native.Context(0)
    c.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    c.set_materials(params.kaist_materials(), s["object_materials"], 0)
    c.set_config(cfg, R.LOOP_ANGLES)
    c.set_beam_samples(golden_beams(R.LOOP_SAMPLES))
    return c, cfg


def test_two_streams_register_different_batches_at_once_beside_a_batch_in_flight(tiles):
    S, T = tiles
    c, cfg = loop_context()
    A = R.LOOP_ANGLES
    poses = np.stack([R.loop_pose((0.1 * k, 0.05 * k, 0.01 * k)) for k in range(8)])
    imgs = torch.zeros((8, cfg.n_cells, A), dtype=torch.uint8, device=DEV)
    work = []
    for seed in (31, 32):
        rs = np.random.RandomState(seed)
        tgt = target_cloud(rs, T + 100)
        clouds = [source_cloud(rs, tgt, m, yaw=0.03) for m in (S + 9, 200, 2 * S)]
        mp = 2 * S
        pts = np.zeros((3, mp), native.POINT_DTYPE)
        offs = np.zeros((3, A + 1), np.uint32)
        for f, cl in enumerate(clouds):
            pts[f, :len(cl)] = R.points_of(cl)
            offs[f, -1] = len(cl)
        b = dict(pts=dev(pts), offs=dev(offs), tgt=dev(R.points_of(tgt)), cnt=dev(np.array([len(tgt)], np.uint32)),
                 rec=torch.zeros(3 * 48, dtype=torch.uint8, device=DEV), corr=torch.zeros(3 * mp * 4, dtype=torch.uint8, device=DEV))
        work.append((b, len(tgt), mp, torch.cuda.Stream(device=DEV)))
    torch.cuda.synchronize()

    def enqueue(b, n_tgt, mp, stream):
        p = {k: v.data_ptr() for k, v in b.items()}
        c.register_points_device(p["pts"], p["offs"], 3, mp, p["tgt"], p["cnt"], n_tgt, p["rec"], None, GATE, 6, p["corr"], stream)

    def results(b):
        return b["rec"].cpu().numpy().tobytes(), b["corr"].cpu().numpy().tobytes()

    c.simulate_batch_device(poses, imgs.data_ptr(), None)             # a batch in flight on the context's stream
    for b, n_tgt, mp, s in work:
        enqueue(b, n_tgt, mp, s.cuda_stream)
    torch.cuda.synchronize()
    c.synchronize()
    together = [results(b) for b, _, _, _ in work]
    busy = imgs.cpu().numpy().copy()
    for b, n_tgt, mp, _ in work:                                     # one after the other, on the context's stream
        b["rec"].zero_(); b["corr"].zero_()
        torch.cuda.synchronize()
        enqueue(b, n_tgt, mp, None)
        c.synchronize()
    assert [results(b) for b, _, _, _ in work] == together and together[0] != together[1]
    imgs.zero_()
    torch.cuda.synchronize()
    c.simulate_batch_device(poses, imgs.data_ptr(), None)
    c.synchronize()
    assert np.array_equal(imgs.cpu().numpy(), busy) and busy.any()   # ... and the batch beside them was not disturbed


# ---- 7. closed loop -----------------------------------------------------------------------------------------------------
def test_closed_loop_the_relative_pose_of_two_scans_of_a_room():
    c, cfg = loop_context()
    imgs = np.stack([c.simulate(R.loop_pose(p))[0] for p in (R.LOOP_A, R.LOOP_B)])
    pts, offs = c.detect(imgs, R.LOOP_DET)
    assert len(pts[0]) >= 100 and len(pts[1]) >= 100
    rec, corr = c.register_points([pts[1]], offs[1:], pts[0], None, R.LOOP_GATE, R.LOOP_ITERATIONS, want_corr=True)
    want, _, want_corr = R.register([pts[1]], pts[0], None, R.LOOP_GATE, R.LOOP_ITERATIONS)
    same_as_ref(rec, None, want, None)
    assert np.array_equal(corr[0], want_corr[0])
    yaw_err, t_err = R.loop_errors(rec[0])
    ident = np.zeros(1, native.ICP_DTYPE)
    ident["c"] = 1.0
    yaw0, t0 = R.loop_errors(ident[0])
    print("closed loop on the GPU: yaw error %.4f deg (identity %.4f), translation error %.4f m (identity %.4f), %d of %d matched"
          % (math.degrees(yaw_err), math.degrees(yaw0), t_err, t0, rec[0]["n_matched"], len(pts[1])))
    assert rec[0]["flags"] == 0 and yaw_err < yaw0 and t_err < t0
    assert yaw_err <= R.LOOP_YAW_BOUND and t_err <= R.LOOP_T_BOUND


def test_radar_facade_register_point_clouds_corrects_the_pose():
    s = R.loop_scene()
    r = radar.RadarHIP(s["verts"], s["faces"], s["face_object_id"])
    r.loadParams(params.kaist_materials(), s["object_materials"], 0)
    r.updateDynCfg(R.loop_cfg())
    r.setBeamSamples(golden_beams(R.LOOP_SAMPLES))
    pose_a, pose_b = R.loop_pose(R.LOOP_A), R.loop_pose(R.LOOP_B)
    real = r.simulatePointClouds(pose_a[None], **R.LOOP_DET)[0]       # the "real" scan: taken at A
    rec, fixed = r.registerPointClouds(np.stack([pose_b, pose_a]), real, detect=R.LOOP_DET, gate=R.LOOP_GATE, iterations=R.LOOP_ITERATIONS)
    assert rec.dtype == native.ICP_DTYPE and fixed.shape == (2, 7) and fixed.dtype == np.float32
    # the hypothesis that is right stays where it is: its cloud is the real cloud
    assert (rec["c"][1], rec["s"][1], rec["tx"][1], rec["ty"][1], rec["sse"][1]) == (1.0, 0.0, 0.0, 0.0, 0) and rec["n_matched"][1] == len(real)
    assert np.allclose(fixed[1], pose_a, atol=1e-6)
    # the record is what the context's host form gives on the same clouds
    cloud_b = r.simulatePointClouds(pose_b[None], **R.LOOP_DET)[0]
    offs = np.zeros((1, 401), np.uint32)
    offs[0, -1] = len(cloud_b)
    assert r.context.register_points([cloud_b], offs, real, None, R.LOOP_GATE, R.LOOP_ITERATIONS)[0].tobytes() == rec[0].tobytes()
    # compensate: an identity sweep table moves no point (rr_compensate_points_device beside the registration), the records are the same bytes
    rec_c, fixed_c = r.registerPointClouds(np.stack([pose_b, pose_a]), real, detect=R.LOOP_DET, gate=R.LOOP_GATE, iterations=R.LOOP_ITERATIONS,
                                           compensate=native.identity_sweep_table(1, 400)[0])
    assert rec_c.tobytes() == rec.tobytes() and fixed_c.tobytes() == fixed.tobytes()
    # ... and a table that moves every point 1 m forward gives what the context's calls give on the moved cloud
    moved = native.identity_sweep_table(1, 400)[0]
    moved["t"][:, 0] = 1.0
    rec_m, _ = r.registerPointClouds(pose_b[None], real, detect=R.LOOP_DET, gate=2.0, iterations=R.LOOP_ITERATIONS, compensate=moved)
    offs_b = np.zeros((1, 401), np.uint32)
    offs_b[0, -1] = len(cloud_b)
    cloud_m = r.context.compensate_points([cloud_b], offs_b, moved[None])
    assert np.allclose(cloud_m[0]["x"], cloud_b["x"] + 1.0, atol=1e-5)
    assert rec_m.tobytes() == r.context.register_points(cloud_m, offs_b, real, None, 2.0, R.LOOP_ITERATIONS).tobytes() != rec[:1].tobytes()
    assert rec_m["tx"][0] < rec["tx"][0]                               # the cloud was moved forward: the way onto the target points further back
    # T = X^-1 X_h: the record is B's planar pose in A, and the corrected pose is A
    yaw_err, t_err = R.loop_errors(rec[0])
    yaw_fixed = 2.0 * math.atan2(float(fixed[0][2]), float(fixed[0][3]))
    d_yaw, d_t = abs(yaw_fixed - R.LOOP_A[2]), math.hypot(float(fixed[0][4]) - R.LOOP_A[0], float(fixed[0][5]) - R.LOOP_A[1])
    print("registerPointClouds: record off the truth by %.4f deg / %.4f m; corrected pose off A by %.4f deg / %.4f m (the hypothesis: %.4f deg / %.4f m)"
          % (math.degrees(yaw_err), t_err, math.degrees(d_yaw), d_t, math.degrees(R.LOOP_B[2]), math.hypot(*R.LOOP_B[:2])))
    assert d_yaw < abs(R.LOOP_B[2]) and d_t < math.hypot(*R.LOOP_B[:2])
    assert d_yaw <= R.LOOP_YAW_BOUND and d_t <= R.LOOP_T_BOUND
    assert abs(float(fixed[0][6]) - float(pose_b[6])) < 1e-6 and abs(float(fixed[0][0])) < 1e-6 and abs(float(fixed[0][1])) < 1e-6     # planar
