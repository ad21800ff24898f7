"""Echo provenance on the GPU (rr_simulate_batch_provenance_device, rr_simulate_provenance, rr_debug_labels): the label kernel alone
against the numpy restatement (tests/labels_ref.py), and the frame path on the nested-box scene of tests/test_labels_host.py, whose
premises that file checks on the oracle: the image is the plain batch's, the exported echo stream is complete and ordered (the
oracle's column step turns it into the GPU's own image column, and it equals the oracle's echo log), every echo names the face,
object, pass and kind it came from, the label planes are the restatement applied to the exported stream."""
import numpy as np
import pytest

import labels_ref as R
import test_labels_host as H
from common import mats_tuple
from radarays_ros_amd import params
from radarays_ros_amd.native import ECHO_SRC_DTYPE, LABEL_NONE, unpack_info

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
A = H.N_ANGLES
STRIDE = 400          # the lane's list holds at most (24 + 48 + 96) * 2 = 336 echoes per azimuth
SENT = 0x5A
# Largest relative deviation of an echo's strength from the oracle's log over the cases of test_stream_equals_the_oracle_log, as
# measured on the MI355X (1.0687e-05).  The chain behind an echo holds up to three Fresnel splits, each of which
# moves with the one-ulp difference of acosf between the GPU's libm and the host's (tests/test_gpu_round6.py), and the wall's BRDF
# raises the cosine of that angle to the 3000th power: an ulp of the angle is some 1e-5 of the strength.  The test allows four times
# the figure; a wrong echo is off by orders of magnitude more.
STRENGTH_REL_DEV = 1.0687e-05


def make_ctx(native_lib, cfg, mesh=True):
    c = native_lib.Context(0)
    if mesh:
        s = H.scene()
        c.set_mesh(s["verts"], s["faces"], s["face_object_id"])
        c.set_materials(H.materials(), s["object_materials"], 0)
    c.set_config(cfg, A)
    c.set_beam_samples(H.beams())
    return c


@pytest.fixture(scope="module")
def ctx(native_lib):
    c = make_ctx(native_lib, H.config())
    yield c
    c.close()


def provenance(c, poses, labels=True, faces=True, echoes=True, stride=STRIDE):
    """one provenance call on device buffers -> (images, labels, faces, echoes [n][A][stride], counts [n][A]) as numpy arrays"""
    poses = np.asarray(poses, np.float32).reshape(-1, 7)
    n, C_ = len(poses), c.cfg.n_cells
    d_img = torch.zeros((n, C_, A), dtype=torch.uint8, device=DEV)
    d_lab = torch.zeros((n, C_, A), dtype=torch.int32, device=DEV) if labels else None
    d_fac = torch.zeros((n, C_, A), dtype=torch.int32, device=DEV) if faces else None
    d_ech = torch.full((n * A * stride * 16 + 64,), SENT, dtype=torch.uint8, device=DEV) if echoes else None
    d_cnt = torch.zeros((n, A), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    c.simulate_batch_provenance_device(poses, d_img.data_ptr(), ptr(d_lab), ptr(d_fac), ptr(d_ech), stride if echoes else 0, d_cnt.data_ptr())
    c.synchronize()
    u32 = lambda t: None if t is None else t.cpu().numpy().view(np.uint32)   # noqa: E731
    raw = None if d_ech is None else d_ech.cpu().numpy()
    ech = None if raw is None else raw[:n * A * stride * 16].view(ECHO_SRC_DTYPE).reshape(n, A, stride)
    if raw is not None:
        assert (raw[n * A * stride * 16:] == SENT).all()
    return d_img.cpu().numpy(), u32(d_lab), u32(d_fac), ech, u32(d_cnt)


def plain(c, poses):
    poses = np.asarray(poses, np.float32).reshape(-1, 7)
    d_img = torch.zeros((len(poses), c.cfg.n_cells, A), dtype=torch.uint8, device=DEV)
    c.simulate_batch_device(poses, d_img.data_ptr())
    c.synchronize()
    return d_img.cpu().numpy()


_RUNS = {}


def run(ctx, n_reflections, rmp, scroll=0, poses=(0,)):
    """the provenance outputs of a config / pose set on the shared context, computed once"""
    key = (n_reflections, bool(rmp), scroll, tuple(poses))
    if key not in _RUNS:
        ctx.set_config(H.config(n_reflections=n_reflections, record_multi_path=rmp, scroll_image=scroll), A)
        _RUNS[key] = provenance(ctx, [H.POSE3[k] for k in poses])
        assert _RUNS[key][4].max() <= STRIDE
    return _RUNS[key]


# ---- 1. k_label alone ---------------------------------------------------------------------------------------------------------------
def src(cells, strs, rs=None, faces=None, infos=None):
    e = np.zeros(len(cells), ECHO_SRC_DTYPE)
    e["cell"], e["strength"] = cells, strs
    e["face"] = np.arange(len(cells)) + 1000 if faces is None else faces
    e["info"] = np.arange(len(cells)) + 7 if infos is None else infos
    if rs is not None:
        e["face"], e["info"] = rs.randint(0, 1 << 30, len(cells)), rs.randint(0, 1 << 29, len(cells))
    return e


def hand_worked(n_cells):
    last = n_cells - 1
    return [src([8], [2.0]), src([8, 8], [2.0, 2.0]), src([8, 8, 8], [2.0, 3.0, 3.0]), src([8, 9], [2.0, 1.0]), src([9, 8], [1.0, 2.0]),
            src([1], [1.0]), src([0], [1.0]), src([last], [1.0]), src([last, 2, last - 1], [1.0, 1.0, 1.0]),
            src([n_cells, n_cells + 1, -1, 1 << 30, -(1 << 31)], [9.0] * 5),
            src([8, 8, 8, 8, 8, 8, 8], [-3.0, 0.0, -0.0, np.inf, -np.inf, np.nan, 1e-30]), src([8, 8, 8], [np.nan, np.inf, -1.0])]


def check_labels(c, oracle, cfg, segs, az_begin=0, stride=None):
    c.set_config(cfg, A)
    w, mode = R.weights(cfg, oracle)
    stride = max(1, max(len(s) for s in segs)) if stride is None else stride
    e = np.zeros((len(segs), stride), ECHO_SRC_DTYPE)
    e["cell"], e["strength"], e["face"], e["info"] = 5, 1e9, 0xDEAD, 0xBEEF          # what lies beyond a count must not be read
    for k, s in enumerate(segs):
        e[k, :len(s)] = s
    lab, fac = c.debug_labels(e, [len(s) for s in segs], az_begin)
    for k, s in enumerate(segs):
        rl, rf = R.label_column_fast(s["cell"], s["strength"], s["info"], s["face"], cfg.n_cells, w, mode)
        assert np.array_equal(lab[k], rl), ("label", k, np.flatnonzero(lab[k] != rl)[:8])
        assert np.array_equal(fac[k], rf), ("face", k, np.flatnonzero(fac[k] != rf)[:8])
    return lab, fac


DEN = {"none": dict(signal_denoising=0), "tri9": dict(signal_denoising=1, signal_denoising_triangular_width=9, signal_denoising_triangular_mode=0.35),
       "tri255": dict(signal_denoising=1, signal_denoising_triangular_width=255, signal_denoising_triangular_mode=0.35)}


@pytest.fixture(scope="module")
def bare(native_lib):
    c = make_ctx(native_lib, H.config(), mesh=False)
    yield c
    c.close()


@pytest.mark.parametrize("n_cells", [64, 65, 512, 3424, 8192])
@pytest.mark.parametrize("den", sorted(DEN))
def test_label_kernel_against_the_restatement(bare, oracle, den, n_cells):
    """hand-worked streams, 3,000 random echoes with many exact ties (strengths from 8 values), odd strengths mixed in, an empty
    segment, a count equal to its stride: both planes, bit for bit.  8,192 cells is the limit the header states."""
    rs = np.random.RandomState(n_cells + len(den))
    cfg = params.RadarModelConfig(n_cells=n_cells, n_reflections=1, ambient_noise=0, **DEN[den])
    ties = src(rs.randint(-2, n_cells + 3, 3000), rs.choice(np.float32([0.25, 0.5, 1.0, 1.5, 2.0, 3.0, 1e-3, 7.0]), 3000), rs)
    close = src(rs.randint(0, min(n_cells, 40), 3000), rs.choice(np.float32([1.0, 1.0 + 2.0 ** -23, 2.0, 0.5]), 3000), rs)
    odd = src(rs.randint(0, n_cells, 300), rs.choice(np.float32([1.0, 2.0, np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0]), 300), rs)
    segs = hand_worked(n_cells) + [ties, close, odd, src([], [])]
    lab, fac = check_labels(bare, oracle, cfg, segs, stride=3000)
    assert (lab[-1] == LABEL_NONE).all() and (fac[-1] == LABEL_NONE).all() and (lab[:, 0] == LABEL_NONE).all()
    assert (lab[len(hand_worked(n_cells))] != LABEL_NONE).sum() > min(n_cells, 3000) // 2


@pytest.mark.parametrize("n_seg,az_begin", [(1, 0), (1, A - 1), (70, 330)])
def test_label_kernel_on_one_and_on_seventy_segments(bare, oracle, n_seg, az_begin):
    rs = np.random.RandomState(n_seg)
    cfg = params.RadarModelConfig(n_cells=512, n_reflections=1, ambient_noise=0, **DEN["tri9"])
    segs = [src(rs.randint(0, 512, n), rs.choice(np.float32([0.5, 1.0, 2.0]), n), rs) for n in rs.randint(0, 200, n_seg)]
    lab, _ = check_labels(bare, oracle, cfg, segs, az_begin=az_begin)
    if n_seg > 1:
        assert len({lab[k].tobytes() for k in range(n_seg)}) > n_seg // 2          # the segments are told apart


# ---- 2. the image -------------------------------------------------------------------------------------------------------------------
def test_image_is_the_plain_batch_and_no_graph_is_involved(native_lib, monkeypatch):
    monkeypatch.setenv("RR_LANES", "1")          # one frame lane: every batch meets the same buffers (and the same graph)
    c = make_ctx(native_lib, H.config())
    want = plain(c, H.POSE3)
    for _ in range(2):
        assert np.array_equal(plain(c, H.POSE3), want)
    cap, rep = c.graph_stats()
    assert cap >= 1 and rep >= 1, (cap, rep)
    img, lab, fac, ech, cnt = provenance(c, H.POSE3)
    assert np.array_equal(img, want)
    assert c.graph_stats() == (cap, rep)
    assert (lab != LABEL_NONE).any() and cnt.min() > 0
    assert np.array_equal(plain(c, H.POSE3), want) and c.graph_stats() == (cap, rep + 1)
    img2 = provenance(c, H.POSE3, labels=False, faces=False, echoes=False)[0]          # the echo counts alone
    assert np.array_equal(img2, want) and not np.array_equal(want[0], want[1])
    c.close()


# ---- 3. the stream is complete and ordered ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rmp", [False, True], ids=["path", "multipath"])
@pytest.mark.parametrize("n_reflections", [1, 3])
def test_stream_through_the_oracle_column_step_gives_the_image(ctx, oracle, n_reflections, rmp):
    """every azimuth's exported (cell, strength) list through orc_column: the GPU's own image column, byte for byte -- the standard
    tests/test_gpu_column.py holds k_column to with the noise off"""
    img, _, _, ech, cnt = run(ctx, n_reflections, rmp)
    cfg = H.config(n_reflections=n_reflections, record_multi_path=rmp)
    for a in range(A):
        e = ech[0, a, :cnt[0, a]]
        _, r8 = oracle.column(cfg, e["cell"], e["strength"], 0.0, a, A)
        assert np.array_equal(img[0][:, a], r8), (a, np.flatnonzero(img[0][:, a] != r8)[:8])
    assert img[0].any()


# ---- 4. against the oracle's log ----------------------------------------------------------------------------------------------------
def test_stream_equals_the_oracle_log(ctx, oracle):
    worst = 0.0
    for pose_index in (0, 1):
        for rmp in (False, True):
            _, _, log = H.logged(oracle, pose_index, 3, rmp)
            _, _, _, ech, cnt = run(ctx, 3, rmp, poses=(pose_index,))
            assert np.array_equal(cnt[0], log["counts"]), (pose_index, rmp, np.flatnonzero(cnt[0] != log["counts"])[:8])
            for a in range(A):
                n = int(cnt[0, a])
                assert np.array_equal(ech[0, a, :n]["cell"], log["cells"][a, :n]), (pose_index, rmp, a)
                g, o = ech[0, a, :n]["strength"].astype(np.float64), log["strengths"][a, :n].astype(np.float64)
                assert np.array_equal(g == 0, o == 0) and np.isfinite(g).all()
                nz = o != 0
                if nz.any():
                    worst = max(worst, float(np.max(np.abs(g[nz] - o[nz]) / np.abs(o[nz]))))
    print("largest relative strength deviation from the oracle's log: %.6g (bound %.6g)" % (worst, 4 * STRENGTH_REL_DEV))
    assert worst <= 4 * STRENGTH_REL_DEV, worst


# ---- 5. provenance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rmp", [False, True], ids=["path", "multipath"])
def test_every_echo_names_its_pass_kind_object_and_face(ctx, oracle, rmp):
    s = H.scene()
    c1, c2, c3 = [H.logged(oracle, 0, P, rmp)[2]["counts"].astype(np.int64) for P in (1, 2, 3)]
    _, _, _, ech, cnt = run(ctx, 3, rmp)
    assert np.array_equal(cnt[0], c3)
    open_az = H.through_the_opening(H.POSE3[0])
    kinds = 0
    for a in range(A):
        e = ech[0, a, :c3[a]]
        obj, pas, kind = unpack_info(e["info"])
        assert (e["info"] >> np.uint32(29) == 0).all()
        want_pass = np.repeat([0, 1, 2], [c1[a], c2[a] - c1[a], c3[a] - c2[a]])
        assert np.array_equal(pas, want_pass), a
        assert (kind[pas == 0] == 0).all() and (rmp or (kind == 0).all()), a
        kinds += int(kind.sum())
        assert (e["face"] < len(s["faces"])).all() and np.array_equal(obj, s["face_object_id"][e["face"]]), a
        p0 = e[:c1[a]]
        near = (p0["cell"] >= H.NEAR_BAND[0]) & (p0["cell"] <= H.NEAR_BAND[1])
        far = (p0["cell"] >= H.FAR_BAND[0]) & (p0["cell"] <= H.FAR_BAND[1])
        assert (near | far).all() and (obj[:c1[a]][near] == 0).all() and (obj[:c1[a]][far] == 1).all(), a
        if open_az[a]:
            assert not (obj[:c1[a]] == 0).any(), a
    assert (kinds > 0) == rmp


# ---- 6. labels from the frame path --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scroll", [0, 37])
def test_label_planes_are_the_restatement_of_the_exported_stream(ctx, oracle, scroll):
    img, lab, fac, ech, cnt = run(ctx, 3, True, scroll=scroll, poses=(0, 1))
    cfg = H.config(n_reflections=3, record_multi_path=True, scroll_image=scroll)
    w, mode = R.weights(cfg, oracle)
    assert len(w) == 9
    for f in range(2):
        rl, rf = R.label_planes(ech[f], cnt[f], cfg.n_cells, w, mode, scroll)
        assert np.array_equal(lab[f], rl), (f, np.argwhere(lab[f] != rl)[:8])
        assert np.array_equal(fac[f], rf), (f, np.argwhere(fac[f] != rf)[:8])
    assert not np.array_equal(lab[0], lab[1]) and (lab[0] != LABEL_NONE).sum() > 10 * A
    obj, pas, kind = unpack_info(lab[0][lab[0] != LABEL_NONE])
    assert set(np.unique(obj)) == {0, 1} and (pas > 0).any()          # both objects and ghosts show in the plane
    # the synchronous host form returns the same frame
    ctx.set_config(cfg, A)
    u8, l1, f1, e1, n1 = ctx.simulate_provenance(H.POSE3[1])
    assert np.array_equal(u8, img[1]) and np.array_equal(l1, lab[1]) and np.array_equal(f1, fac[1]) and np.array_equal(n1, cnt[1])
    for a in range(A):
        assert np.array_equal(e1[a, :n1[a]], ech[1, a, :n1[a]]), a


# ---- 7. truncation and refusals ---------------------------------------------------------------------------------------------------
def test_a_short_echo_stride_truncates_the_rows_and_keeps_the_counts(ctx):
    _, _, _, full, cnt = run(ctx, 3, True)
    ctx.set_config(H.config(n_reflections=3, record_multi_path=True), A)
    stride = (int(cnt.min()) + int(cnt.max())) // 2          # some rows are cut, some are not
    assert cnt.max() > stride >= cnt.min()
    _, _, _, ech, cnt2 = provenance(ctx, [H.POSE3[0]], labels=False, faces=False, stride=stride)          # (checks the tail guard itself)
    assert np.array_equal(cnt2, cnt)
    sentinel = np.full(1, SENT, np.uint8).repeat(16).view(ECHO_SRC_DTYPE)[0]
    for a in range(A):
        m = min(int(cnt[0, a]), stride)
        assert np.array_equal(ech[0, a, :m], full[0, a, :m]), a
        assert (ech[0, a, m:] == sentinel).all(), a
    # the host form: true counts, the first `stride` records, nothing beyond them
    L = ctx._L
    he = np.full((A, stride + 1), sentinel, ECHO_SRC_DTYPE)
    hc = np.zeros(A, np.uint32)
    u8 = np.zeros((512, A), np.uint8)
    pose = np.ascontiguousarray(H.POSE3[0], np.float32)
    assert L.rr_simulate_provenance(ctx._h, pose.ctypes.data, u8.ctypes.data, None, None, he.ctypes.data, stride + 1, hc.ctypes.data) == 0
    assert np.array_equal(hc, cnt[0])
    for a in range(A):
        m = min(int(cnt[0, a]), stride + 1)
        assert np.array_equal(he[a, :m], full[0, a, :m]) and (he[a, m:] == sentinel).all(), a


def test_refusals_write_nothing(native_lib, bare):
    L = native_lib.lib()
    pose = np.ascontiguousarray(np.tile(H.POSE3[0], (65, 1)), np.float32)
    n_cells = 512
    d = {k: torch.full((n_cells * A * 4 + 64,), SENT, dtype=torch.uint8, device=DEV) for k in ("img", "lab", "fac", "ech", "cnt")}
    host = {k: np.full(n_cells * A * 4, SENT, np.uint8) for k in ("img", "lab", "fac", "ech", "cnt")}
    torch.cuda.synchronize()

    def dev_call(c, poses=pose.ctypes.data, n=1, img=True, ech=True, cnt=True, stride=4):
        p = lambda k, on: d[k].data_ptr() if on else None   # noqa: E731
        return L.rr_simulate_batch_provenance_device(c._h, poses, n, p("img", img), p("lab", True), p("fac", True), p("ech", ech), stride, p("cnt", cnt), None)

    def host_call(c, poses=pose.ctypes.data, img=True, ech=True, cnt=True, stride=4):
        p = lambda k, on: host[k].ctypes.data if on else None   # noqa: E731
        return L.rr_simulate_provenance(c._h, poses, p("img", img), p("lab", True), p("fac", True), p("ech", ech), stride, p("cnt", cnt))

    def untouched(c):
        c.synchronize()
        return all((t.cpu().numpy() == SENT).all() for t in d.values()) and all((h == SENT).all() for h in host.values())

    # -2: no mesh (the context of the label-kernel tests), no config
    assert dev_call(bare) == -2 and host_call(bare) == -2 and "rr_set_mesh" in L.rr_last_error(bare._h).decode()
    fresh = native_lib.Context(0)
    lab = np.full(8, SENT, np.uint32)
    one = np.ones(1, np.uint32)
    e = np.zeros(4, ECHO_SRC_DTYPE)
    assert L.rr_debug_labels(fresh._h, 1, 0, e.ctypes.data, one.ctypes.data, 4, lab.ctypes.data, lab.ctypes.data) == -2
    assert dev_call(fresh) == -2 and untouched(fresh)
    fresh.close()
    # -3: the arguments
    c = make_ctx(native_lib, H.config())
    bad = [dict(poses=None), dict(img=False), dict(n=0), dict(n=65), dict(cnt=False), dict(stride=0)]
    for kw in bad:
        assert dev_call(c, **kw) == -3, kw
        assert "rr_simulate_batch_provenance_device" in L.rr_last_error(c._h).decode(), kw
        if "n" not in kw:
            assert host_call(c, **kw) == -3, kw
    # an n_cells the LDS column cannot hold never gets as far as a provenance call: RR_LABEL_MAX_CELLS is the most rr_set_config admits
    with pytest.raises(native_lib.RRError, match="n_cells.*rc=-3"):
        c.set_config(params.RadarModelConfig(n_cells=native_lib.LABEL_MAX_CELLS + 1, n_reflections=1, ambient_noise=0), A)
    c.set_config(params.RadarModelConfig(n_cells=native_lib.LABEL_MAX_CELLS, n_reflections=1, ambient_noise=0), A)
    with pytest.raises(native_lib.RRError, match="n_reflections.*rc=-3"):          # ... and so does a pass the info word cannot hold
        c.set_config(H.config(n_reflections=17), A, max_waves_per_azimuth=64)
    assert untouched(c)
    c.close()
    # rr_debug_labels: a count above its stride, a block outside the image, null buffers
    bare.set_config(H.config(), A)
    S32 = SENT * 0x01010101
    lab, fac = np.full(512, S32, np.uint32), np.full(512, S32, np.uint32)
    five = np.full(1, 5, np.uint32)
    args = lambda **kw: [kw.get("n_seg", 1), kw.get("az", 0), e.ctypes.data, kw.get("cnt", one.ctypes.data), 4, kw.get("lab", lab.ctypes.data), fac.ctypes.data]   # noqa: E731
    for kw in (dict(cnt=five.ctypes.data), dict(n_seg=0), dict(az=A), dict(az=-1), dict(cnt=None), dict(lab=None)):
        assert L.rr_debug_labels(bare._h, *args(**kw)) == -3, kw
        assert "rr_debug_labels" in L.rr_last_error(bare._h).decode()
    assert (lab == S32).all() and (fac == S32).all()
    assert L.rr_debug_labels(bare._h, *args()) == 0 and (lab != S32).all()


# ---- 8. dynamic scene ---------------------------------------------------------------------------------------------------------------
def test_a_moved_object_keeps_its_provenance(native_lib):
    s = H.scene()
    c = make_ctx(native_lib, H.config(n_reflections=3, record_multi_path=True))
    _, lab0, fac0, ech0, cnt0 = provenance(c, [H.POSE3[0]])
    c.set_object_poses([[0, 0, 0, 1, 1.0, 0, 0], [0, 0, 0, 1, 0, 0, 0]])          # object 0 moves 1 m along x
    _, lab1, fac1, ech1, cnt1 = provenance(c, [H.POSE3[0]])
    for ech, cnt in ((ech0, cnt0), (ech1, cnt1)):
        for a in range(A):
            e = ech[0, a, :cnt[0, a]]
            assert (e["face"] < len(s["faces"])).all() and np.array_equal(unpack_info(e["info"])[0], s["face_object_id"][e["face"]]), a
    assert not np.array_equal(lab0, lab1)
    # the wall behind the sensor came 1 m closer: the nearest labelled cell of object 0 moved from 5 m to 4 m
    def nearest(lab):
        rows = np.flatnonzero(((lab[0] != LABEL_NONE) & (unpack_info(lab[0])[0] == 0)).any(axis=1))
        return int(rows.min())
    assert nearest(lab0) in range(95, 101) and nearest(lab1) in range(75, 81)
    c.close()
