"""Wave paths on the GPU (rr_simulate_batch_paths_device, rr_simulate_paths): every azimuth's list of ray-cast waves held to its own
definition (include/radarays_mi355.h), to the provenance stream of the same pose, to the restatement of the bounce loop
(tests/paths_ref.py, which tests/test_paths_host.py pins to the oracle) and to itself under other launch shapes.  The cases are those
of tests/test_paths_host.py, which proves their premises on the oracle alone: single passes of more than 256 and of more than 512
waves (second and third sweep of the gather), waves with both echoes, misses, no energy near the pruning threshold."""
import numpy as np
import pytest

import paths_ref as R
import test_paths_host as H
from radarays_ros_amd import radar
from radarays_ros_amd.native import WAVE_DTYPE, WAVES_MAP_FRAME, RRError
from test_gpu_dynamic import posed_soup
from test_gpu_labels import plain, provenance

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
A = H.N_ANGLES
SENT = 0x5A
NP = 16
# Largest relative deviation of a later-pass wave's o / d / range / energy / time from the restatement per case, over the azimuths of
# tests/test_paths_host.py, as measured on the MI355X (with the wave that set it).  The source is the one
# tests/test_gpu_labels.py states for its STRENGTH_REL_DEV: one ulp of acosf per Fresnel split between the GPU's libm and the host's
# ("Arithmetic fidelity").  The test allows four times the figure.
REL_DEV = {"N": 7.267074e-07, "A": 3.531164e-06, "B": 1.177102e-06, "B2": 1.253596e-06}


def make_ctx(native_lib, case, rmp=True, builder="host", scene=None):
    c = native_lib.Context(0)
    s = H.scene(case) if scene is None else scene
    c.set_mesh(s["verts"], s["faces"], s["face_object_id"], builder=builder)
    c.set_materials(H.materials(case), s["object_materials"], 0)
    c.set_config(H.config(case, rmp), A)
    c.set_beam_samples(H.beams(case))
    return c


@pytest.fixture(scope="module")
def ctxs(native_lib):
    cs = {k: make_ctx(native_lib, k) for k in ("N", "A", "B")}
    cs["B2"] = cs["B"]
    yield cs
    for k in ("N", "A", "B"):
        cs[k].close()


def paths(c, poses, stride, flags=0, waves=True, stream=None, sync=True):
    """one paths call on device buffers -> (images, records [n][A][stride], counts [n][A], pass counts [n][A][16]); the bytes behind
    the last row are checked to be untouched"""
    poses = np.asarray(poses, np.float32).reshape(-1, 7)
    n = len(poses)
    d_img = torch.zeros((n, c.cfg.n_cells, A), dtype=torch.uint8, device=DEV)
    d_wav = torch.full((n * A * stride * 64 + 64,), SENT, dtype=torch.uint8, device=DEV) if waves else None
    d_cnt = torch.full((n, A), -1, dtype=torch.int32, device=DEV)
    d_pc = torch.full((n, A, NP), -1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    c.simulate_batch_paths_device(poses, d_img.data_ptr(), d_wav.data_ptr() if waves else None, stride if waves else 0, d_cnt.data_ptr(),
                                  d_pc.data_ptr(), flags, stream)
    out = (d_img, d_wav, d_cnt, d_pc, n, stride)
    return fetch(c, out) if sync else out


def fetch(c, out):
    d_img, d_wav, d_cnt, d_pc, n, stride = out
    c.synchronize()
    raw = None if d_wav is None else d_wav.cpu().numpy()
    rec = None if raw is None else raw[:n * A * stride * 64].view(WAVE_DTYPE).reshape(n, A, stride)
    if raw is not None:
        assert (raw[n * A * stride * 64:] == SENT).all()
    return d_img.cpu().numpy(), rec, d_cnt.cpu().numpy().view(np.uint32).astype(np.int64), d_pc.cpu().numpy().view(np.uint32).astype(np.int64)


def written(rec, cnt):
    """the records that exist, as bytes per azimuth (what lies behind a count is the caller's own)"""
    return [rec[a, :cnt[a]].tobytes() for a in range(A)]


def same_lists(x, y):
    (_, ra, ca, pa), (_, rb, cb, pb) = x, y
    assert np.array_equal(ca, cb) and np.array_equal(pa, pb)
    for f in range(len(ca)):
        assert written(ra[f], ca[f]) == written(rb[f], cb[f]), f


_RUNS = {}


def run(ctxs, case, rmp):
    """(image, records [A][stride], counts [A], pass counts [A][16], stats) of one case on the shared context, computed once"""
    if (case, rmp) not in _RUNS:
        c = ctxs[case]
        c.set_config(H.config(case, rmp), A)
        img, rec, cnt, pc = paths(c, [H.pose(case)], H.STRIDE[case])
        st = c.stats()
        for v in (img, rec, cnt, pc):
            v.setflags(write=False)
        _RUNS[(case, rmp)] = (img[0], rec[0], cnt[0], pc[0], st)
    return _RUNS[(case, rmp)]


# ---- 1. the lists against their definition ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,rmp", H.RUNS, ids=H.IDS)
def test_lists_are_consistent_with_themselves(ctxs, case, rmp):
    _, rec, cnt, pc, st = run(ctxs, case, rmp)
    P = H.n_passes(case)
    assert cnt.max() <= H.STRIDE[case] and cnt.sum() == st["wave_passes"], (cnt.sum(), st)
    assert np.array_equal(pc.sum(1), cnt) and (pc[:, P:] == 0).all() and (pc[:, 0] == len(H.beams(case))).all()
    beams = np.asarray(H.beams(case), np.float32).reshape(-1, 3)
    hits = 0
    skip = np.float64(np.float32(0.001))
    for a in range(A):
        w = rec[a, :cnt[a]]
        H.check_list(w, pc[a, :P], int((radar.unpack_wave_info(w["info"])[3].astype(np.int64) + radar.unpack_wave_info(w["info"])[4]).sum()))
        hits += int((w["range"] >= 0).sum())
        b = w[:pc[a, 0]]
        assert not b["o"].view(np.uint32).any() and np.array_equal(b["d"].view(np.uint32), beams.view(np.uint32))
        assert (b["energy"] == 1.0).all() and (b["time"] == 0.0).all()
        ch = w[pc[a, 0]:]
        p = w[ch["parent"]]
        assert np.array_equal(ch["time"], (p["time"] + p["range"].astype(np.float64) / 0.3) + skip / 0.3)       # move, then move by skip_dist: f64, exact
        # child.o = fl(fl(o + fl(d * range)) + fl(d' * skip)) per component, four roundings of relative size u = 2^-24 each: against the
        # exact value the error is at most u * (|d * range| + |o + d * range| + |d' * skip| + |child.o|), with second-order terms
        # (u^2) covered by the factor 1 + 2^-20
        o, d, r, dc = p["o"].astype(np.float64), p["d"].astype(np.float64), p["range"].astype(np.float64)[:, None], ch["d"].astype(np.float64)
        exact = o + d * r + dc * skip
        bound = 2.0 ** -24 * (np.abs(d * r) + np.abs(o + d * r) + np.abs(dc * skip) + np.abs(ch["o"].astype(np.float64))) * (1 + 2.0 ** -20)
        assert (np.abs(ch["o"] - exact) <= bound).all(), (a, np.argwhere(np.abs(ch["o"] - exact) > bound)[:4])
        assert (ch["energy"] > float(np.float32(0.001))).all()          # pruned at the threshold
    assert hits == st["hits"], (hits, st)


# ---- 2. against the provenance stream -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,rmp", H.RUNS, ids=H.IDS)
def test_echo_indices_name_the_provenance_stream(ctxs, case, rmp):
    img, rec, cnt, _, _ = run(ctxs, case, rmp)
    c = ctxs[case]
    c.set_config(H.config(case, rmp), A)
    estride = 2 * H.STRIDE[case]
    pimg, _, _, ech, ecnt = provenance(c, [H.pose(case)], labels=False, faces=False, stride=estride)
    assert np.array_equal(pimg[0], img) and ecnt.max() <= estride
    both = 0
    for a in range(A):
        w = rec[a, :cnt[a]]
        obj, pas, _, e0, e1 = radar.unpack_wave_info(w["info"])
        n = int(ecnt[0, a])
        face, info = np.full(n, 0xFFFFFFFF, np.uint32), np.full(n, 0xFFFFFFFF, np.uint32)
        i0, i1 = w["echo"][e0 > 0], (w["echo"] + e0.astype(np.int32))[e1 > 0]
        assert len(i0) + len(i1) == n and len(np.unique(np.concatenate([i0, i1]))) == n and (n == 0 or max(i0.max(initial=-1), i1.max(initial=-1)) == n - 1)
        face[i0], info[i0] = w["face"][e0 > 0], (obj | pas << np.uint32(24))[e0 > 0]
        face[i1], info[i1] = w["face"][e1 > 0], (obj | pas << np.uint32(24) | np.uint32(1 << 28))[e1 > 0]
        assert np.array_equal(ech[0, a, :n]["face"], face) and np.array_equal(ech[0, a, :n]["info"], info), a
        both += int((e0 & e1).sum())
    assert rmp or both == 0          # (that such waves exist: tests/test_paths_host.py, premise (c))


def test_image_is_the_plain_batch_and_no_graph_is_involved(native_lib, monkeypatch):
    monkeypatch.setenv("RR_LANES", "1")          # one frame lane: every batch meets the same buffers (and the same graph)
    c = make_ctx(native_lib, "N")
    poses = H.L.POSE3
    want = plain(c, poses)
    for _ in range(2):
        assert np.array_equal(plain(c, poses), want)
    cap, rep = c.graph_stats()
    assert cap >= 1 and rep >= 1, (cap, rep)
    img, rec, cnt, pc = paths(c, poses, H.STRIDE["N"])
    assert np.array_equal(img, want) and cnt.min() > 0 and c.graph_stats() == (cap, rep)
    assert np.array_equal(plain(c, poses), want) and c.graph_stats() == (cap, rep + 1)
    img2, _, cnt2, _ = paths(c, poses, 0, waves=False)          # the counts alone
    assert np.array_equal(img2, want) and np.array_equal(cnt2, cnt) and not np.array_equal(want[0], want[1])
    c.close()


# ---- 3. against the restatement ---------------------------------------------------------------------------------------------------
def rel_dev(got, ref):
    """largest relative deviation of the later-pass waves: vectors by their largest component, scalars by their value -> (figure, wave, field)"""
    worst = (0.0, -1, "")
    for f in ("o", "d", "range", "energy", "time"):
        g, r = got[f].astype(np.float64), ref[f].astype(np.float64)
        if g.ndim == 2:
            dev = np.abs(g - r).max(1) / np.abs(r).max(1)
        else:
            dev = np.where(r == g, 0.0, np.abs(g - r) / np.maximum(np.abs(r), 1e-300))
        k = int(np.argmax(dev)) if len(dev) else -1
        if k >= 0 and dev[k] > worst[0]:
            worst = (float(dev[k]), k, f)
    return worst


@pytest.mark.parametrize("case,rmp", H.RUNS, ids=H.IDS)
def test_records_against_the_restatement(ctxs, oracle, case, rmp):
    """exact: waves per pass, parent, branch, material, face, object, echo flags and index, and everything of pass 0; later-pass o, d,
    range, energy and time within four times the deviation measured for the case"""
    _, rec, cnt, pc, _ = run(ctxs, case, rmp)
    worst = (0.0, -1, "", -1)
    for az in H.AZS:
        ref, rpc, _ = H.reference(oracle, case, rmp, az)
        got = rec[az, :cnt[az]]
        assert np.array_equal(pc[az, :len(rpc)], rpc), (case, az, pc[az], rpc)
        for f in ("parent", "material", "face", "info", "echo"):
            bad = np.flatnonzero(got[f] != ref[f])
            assert bad.size == 0, (case, az, f, bad[:4], got[f][bad[:4]], ref[f][bad[:4]])
        n0 = int(rpc[0])
        assert got[:n0].tobytes() == ref[:n0].tobytes(), (case, az, "pass 0")
        dev, k, f = rel_dev(got[n0:], ref[n0:])
        if dev > worst[0]:
            worst = (dev, n0 + k, f, az)
    print("paths rel dev %s %s: %.6e (azimuth %d, wave %d, %s)" % (case, "multipath" if rmp else "path", worst[0], worst[3], worst[1], worst[2]))
    assert worst[0] <= 4 * REL_DEV[case], (case, worst)


# ---- 4. the map frame ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["N", "A"])
def test_map_frame_moves_only_o_and_d(ctxs, oracle, case):
    _, rec, cnt, pc, _ = run(ctxs, case, True)
    c = ctxs[case]
    c.set_config(H.config(case, True), A)
    pose = np.asarray(H.pose(case), np.float32)
    _, mrec, mcnt, mpc = paths(c, [pose], H.STRIDE[case], flags=WAVES_MAP_FRAME)
    assert np.array_equal(mcnt[0], cnt) and np.array_equal(mpc[0], pc)
    for a in range(A):
        s, m = rec[a, :cnt[a]], mrec[0, a, :cnt[a]]
        for f in WAVE_DTYPE.names:
            if f not in ("o", "d"):
                assert s[f].tobytes() == m[f].tobytes(), (a, f)
        n0 = pc[a, 0]
        assert np.array_equal(m["o"][:n0].view(np.uint32), np.broadcast_to(pose[4:], (n0, 3)).view(np.uint32))
    for a in H.AZS:      # the rotation in numpy f32, the kernel's operation order up to the products by the zero w: a few ulps of a unit vector
        q_am, t_am = R.azimuth_frame(pose, a, oracle.make_config(c.cfg, A))
        s, m = rec[a, :cnt[a]], mrec[0, a, :cnt[a]]
        d = np.stack(R.q_rot(q_am, tuple(s["d"][:, k] for k in range(3))), 1)
        o = np.stack(R.v_add(R.q_rot(q_am, tuple(s["o"][:, k] for k in range(3))), t_am), 1)
        assert np.abs(m["d"] - d).max() <= 4 * 2.0 ** -24
        later = slice(pc[a, 0], None)
        assert (np.abs(m["o"][later] - o[later]) <= 4 * 2.0 ** -24 * np.maximum(np.abs(o[later]).max(1, keepdims=True), np.abs(s["o"][later]).max(1, keepdims=True))).all()


# ---- 5. invariance, GPU against GPU -----------------------------------------------------------------------------------------------
def test_position_in_a_batch_of_eight(ctxs):
    c = ctxs["N"]
    c.set_config(H.config("N", True), A)
    poses = [H.L.POSE3[k % 3] for k in range(8)]
    out = paths(c, poses, H.STRIDE["N"])
    for k in range(3):
        one = paths(c, [H.L.POSE3[k]], H.STRIDE["N"])
        for f in range(k, 8, 3):
            assert np.array_equal(out[0][f], one[0][0]) and np.array_equal(out[2][f], one[2][0]) and np.array_equal(out[3][f], one[3][0])
            assert written(out[1][f], out[2][f]) == written(one[1][0], one[2][0]), (k, f)
    assert written(out[1][0], out[2][0]) != written(out[1][1], out[2][1])


@pytest.mark.parametrize("how", ["gpu_builder", "full_rows"])
def test_tree_builder_and_trace_rows_change_no_record(ctxs, native_lib, monkeypatch, how):
    base = run(ctxs, "A", True)
    if how == "full_rows":
        monkeypatch.setenv("RR_TIGHT_GRID", "0")
    c = make_ctx(native_lib, "A", builder="gpu" if how == "gpu_builder" else "host")
    for _ in range(2):      # the second batch runs with the rows the first one's history asks for
        img, rec, cnt, pc = paths(c, [H.pose("A")], H.STRIDE["A"])
        assert np.array_equal(img[0], base[0]) and np.array_equal(cnt[0], base[2]) and np.array_equal(pc[0], base[3])
        assert written(rec[0], cnt[0]) == written(base[1], base[2])
    c.close()


def test_moved_object_equals_a_fresh_context_of_the_posed_soup(native_lib):
    s = H.scene("N")
    poses = np.float32([[0, 0, np.sin(0.2), np.cos(0.2), 0.3, -0.2, 0.1], [0, 0, 0, 1, 0, 0, 0]])
    c = make_ctx(native_lib, "N")
    c.set_object_poses(poses)
    moved = paths(c, [H.pose("N")], H.STRIDE["N"])
    d = make_ctx(native_lib, "N", scene=posed_soup(s, poses))
    fresh = paths(d, [H.pose("N")], H.STRIDE["N"])
    e = make_ctx(native_lib, "N")
    rest = paths(e, [H.pose("N")], H.STRIDE["N"])
    assert np.array_equal(moved[0], fresh[0])
    same_lists(moved, fresh)
    assert written(moved[1][0], moved[2][0]) != written(rest[1][0], rest[2][0])
    for x in (c, d, e):
        x.close()


def test_include_motion_with_a_pose_table(native_lib):
    """a table that holds the same pose for every azimuth is the plain call; a table of its own changes the lists, and the map-frame
    start points of pass 0 are the table's translations"""
    c = make_ctx(native_lib, "N")
    pose = np.asarray(H.pose("N"), np.float32)
    base = paths(c, [pose], H.STRIDE["N"])
    c.set_motion_poses(np.broadcast_to(pose, (A, 7)).copy())
    same_lists(paths(c, [H.L.POSE3[1]], H.STRIDE["N"]), base)          # the call's own pose is not looked at
    table = np.broadcast_to(pose, (A, 7)).copy()
    table[:, 4] += np.linspace(0.0, 0.5, A, dtype=np.float32)
    c.set_motion_poses(table)
    _, rec, cnt, pc = paths(c, [pose], H.STRIDE["N"], flags=WAVES_MAP_FRAME)
    assert written(rec[0], cnt[0]) != written(base[1][0], base[2][0])
    for a in range(A):
        assert np.array_equal(rec[0, a, :pc[0, a, 0]]["o"].view(np.uint32), np.broadcast_to(table[a, 4:], (pc[0, a, 0], 3)).view(np.uint32))
    c.close()


# ---- 6. truncation and refusals -----------------------------------------------------------------------------------------------------
def test_short_rows_keep_true_counts_and_indices(ctxs):
    _, rec, cnt, pc, _ = run(ctxs, "A", True)
    c = ctxs["A"]
    c.set_config(H.config("A", True), A)
    short = 700          # inside pass 1 of every azimuth (300 + 600 waves)
    assert short < cnt.min()
    _, srec, scnt, spc = paths(c, [H.pose("A")], short)          # (paths() checks the guard bytes behind the last row)
    assert np.array_equal(scnt[0], cnt) and np.array_equal(spc[0], pc)
    assert srec[0].tobytes() == np.ascontiguousarray(rec[:, :short]).tobytes()
    # the host call: rows longer than a list can get, and shorter than the lists
    u8, hrec, hcnt, hpc = c.simulate_paths(H.pose("A"), wave_stride=short)
    assert np.array_equal(hcnt, cnt) and np.array_equal(hpc, pc) and hrec.tobytes() == srec[0].tobytes()


def test_host_call_sizes_its_rows(ctxs):
    img, rec, cnt, pc, _ = run(ctxs, "N", True)
    c = ctxs["N"]
    c.set_config(H.config("N", True), A)
    u8, hrec, hcnt, hpc = c.simulate_paths(H.pose("N"))
    assert np.array_equal(u8, img) and np.array_equal(hcnt, cnt) and np.array_equal(hpc, pc) and hrec.shape == (A, cnt.max())
    assert written(hrec, hcnt) == written(rec, cnt)
    big = c.simulate_paths(H.pose("N"), wave_stride=100000)[1]          # longer than a list can get: the device row is capped
    assert written(big, hcnt) == written(rec, cnt) and not big[:, cnt.max():].view(np.uint8).any()
    assert c.simulate_paths(H.pose("N"), wave_stride=0)[1] is None


def test_refusals_write_nothing(ctxs, native_lib):
    c = ctxs["N"]
    c.set_config(H.config("N", True), A)
    Lb, h = native_lib.lib(), c._h
    pose = np.asarray(H.pose("N"), np.float32)
    buf = torch.full((4096,), SENT, dtype=torch.uint8, device=DEV)
    img, wav, cn = buf.data_ptr(), buf.data_ptr() + 1024, buf.data_ptr() + 2048
    calls = [((None, 1, img, wav, 1, cn, None, 0, None), "null poses/output"), ((pose.ctypes.data, 1, None, wav, 1, cn, None, 0, None), "null poses/output"),
             ((pose.ctypes.data, 1, img, wav, 1, None, None, 0, None), "needs a count buffer"), ((pose.ctypes.data, 1, img, wav, 0, cn, None, 0, None), "wave_stride must be positive"),
             ((pose.ctypes.data, 0, img, wav, 1, cn, None, 0, None), "n_frames must be 1..64"), ((pose.ctypes.data, 65, img, wav, 1, cn, None, 0, None), "n_frames must be 1..64"),
             ((pose.ctypes.data, 1, img, wav, 1, cn, None, 2, None), "unknown flag bits"), ((pose.ctypes.data, 1, img, wav + 4, 1, cn, None, 0, None), "16-byte aligned")]
    for args, msg in calls:
        assert Lb.rr_simulate_batch_paths_device(h, *args) == -3 and msg in Lb.rr_last_error(h).decode(), (args, Lb.rr_last_error(h))
    hw, hc, h8 = np.full(64, SENT, np.uint8), np.full(4 * A, SENT, np.uint8), np.full(c.cfg.n_cells * A, SENT, np.uint8)
    assert Lb.rr_simulate_paths(h, pose.ctypes.data, h8.ctypes.data, hw.ctypes.data, 1, None, None, 0) == -3 and "needs a count buffer" in Lb.rr_last_error(h).decode()
    assert Lb.rr_simulate_paths(h, pose.ctypes.data, h8.ctypes.data, hw.ctypes.data, 0, hc.ctypes.data, None, 0) == -3
    assert Lb.rr_simulate_paths(h, pose.ctypes.data, h8.ctypes.data, None, 0, hc.ctypes.data, None, 4) == -3 and "unknown flag bits" in Lb.rr_last_error(h).decode()
    assert Lb.rr_simulate_paths(h, None, h8.ctypes.data, None, 0, hc.ctypes.data, None, 0) == -3
    bare = native_lib.Context(0)
    assert Lb.rr_simulate_batch_paths_device(bare._h, pose.ctypes.data, 1, img, wav, 1, cn, None, 0, None) == -2 and Lb.rr_last_error(bare._h)
    bare.set_config(H.config("N", True), A)
    assert Lb.rr_simulate_batch_paths_device(bare._h, pose.ctypes.data, 1, img, wav, 1, cn, None, 0, None) == -2          # no mesh
    bare.close()
    c.synchronize()
    assert (buf.cpu().numpy() == SENT).all() and (hw == SENT).all() and (hc == SENT).all() and (h8 == SENT).all()
    with pytest.raises(RRError):
        c.simulate_batch_paths_device(pose, img, wav, 1, None)


def test_no_pass_gives_no_wave(native_lib):
    c = make_ctx(native_lib, "N")
    c.set_config(H.L.config(0, True), A)
    img, rec, cnt, pc = paths(c, [H.pose("N")], 4)
    assert not cnt.any() and not pc.any() and not img.any() and (rec.view(np.uint8) == SENT).all()
    u8, hrec, hcnt, hpc = c.simulate_paths(H.pose("N"))
    assert not hcnt.any() and not hpc.any() and hrec.shape == (A, 1)
    c.close()


# ---- 7. two calls in flight ---------------------------------------------------------------------------------------------------------
def test_two_calls_on_different_lanes(ctxs):
    c = ctxs["N"]
    c.set_config(H.config("N", True), A)
    singles = [paths(c, [H.L.POSE3[k]], H.STRIDE["N"]) for k in (0, 1)]
    pending = [paths(c, [H.L.POSE3[k]], H.STRIDE["N"], sync=False) for k in (0, 1)]          # consecutive calls take consecutive lanes
    for k in (0, 1):
        got = fetch(c, pending[k])
        assert np.array_equal(got[0], singles[k][0])
        same_lists(got, singles[k])
    assert written(singles[0][1][0], singles[0][2][0]) != written(singles[1][1][0], singles[1][2][0])
