"""Connected components on the GPU: rr_label_components_device equals the numpy restatement (tests/components_ref.py) byte for byte -- labels,
cleaned plane, records and counts -- on every case of the shared list; writes nothing outside what it owns; does not depend on what the
scratch held or on an earlier call; the host form, the facades and the C++ mirror give the same bytes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import components_ref as R
import field_ref as F
import icp_ref
from common import golden_beams
from radarays_ros_amd import native, params, radar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, FILL = 256, 0xA5
REC = native.COMPONENT_DTYPE.itemsize


@pytest.fixture(scope="module")
def ctx():
    return native.Context(0)


@pytest.fixture(scope="module")
def cases():
    return R.all_cases(*native.components_tile_sizes())


@pytest.fixture(scope="module")
def wants(cases):
    """the restatement's answer to every case, computed once"""
    return [R.label_case(c) for c in cases]


def cfg_of(c, **kw):
    _, H, W = c["planes"].shape
    a = dict(threshold=c["threshold"], connectivity=c["connectivity"], wrap_x=c["wrap_x"], min_pixels=c["min_pixels"], max_components=c["max_components"])
    a.update(kw)
    return native.components_config(H, W, **a)


class Guarded:
    """`nbytes` bytes of HBM between two guards, all filled with FILL (or with seeded noise)"""

    def __init__(self, nbytes, noise=None):
        self.n = int(nbytes)
        if noise is None:
            self.t = torch.full((self.n + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
        else:
            self.t = torch.from_numpy(np.random.default_rng(noise).integers(0, 256, self.n + 2 * GUARD, dtype=np.uint8)).cuda()
            self.t[:GUARD] = FILL
            self.t[GUARD + self.n:] = FILL
        self.ptr = self.t.data_ptr() + GUARD

    def body(self):
        return self.t[GUARD:GUARD + self.n].cpu().numpy()

    def guards_intact(self):
        h = self.t.cpu().numpy()
        return bool((h[:GUARD] == FILL).all() and (h[GUARD + self.n:] == FILL).all())


def run(ctx, c, g=None, labels=True, clean=True, scratch_noise=None, scratch=None):
    """the device form on guarded buffers -> dict(labels, clean, comps (a list per plane), counts, tail (the untouched records' bytes))"""
    g = g or cfg_of(c)
    planes = c["planes"]
    n, npx = len(planes), planes[0].size
    d_planes = torch.from_numpy(planes).cuda()
    need = ctx.components_scratch_bytes(n, g)
    B = dict(counts=Guarded(8 * n), scratch=scratch or Guarded(need, scratch_noise))
    if labels:
        B["labels"] = Guarded(4 * n * npx)
    if clean:
        B["clean"] = Guarded(n * npx)
    if g.max_components:
        B["comps"] = Guarded(n * g.max_components * REC)
    ptr = lambda k: B[k].ptr if k in B else None      # noqa: E731
    ctx.label_components_device(d_planes.data_ptr(), n, g, ptr("labels"), ptr("clean"), ptr("comps"), ptr("counts"), ptr("scratch"), B["scratch"].n)
    ctx.synchronize()
    for k, b in B.items():
        assert b.guards_intact(), (c["label"], k)
    assert np.array_equal(d_planes.cpu().numpy(), planes)
    out = dict(counts=B["counts"].body().view(np.uint32).reshape(n, 2), scratch=B["scratch"])
    if labels:
        out["labels"] = B["labels"].body().view(np.uint32).reshape(planes.shape)
    if clean:
        out["clean"] = B["clean"].body().reshape(planes.shape)
    out["comps"], out["tail_untouched"] = [], True
    for a in range(n):
        k = min(int(out["counts"][a, 0]), g.max_components)
        if g.max_components:
            raw = B["comps"].body().reshape(n, g.max_components * REC)[a]
            out["comps"].append(raw[:k * REC].view(native.COMPONENT_DTYPE).copy())
            out["tail_untouched"] &= bool((raw[k * REC:] == FILL).all())
        else:
            out["comps"].append(np.zeros(0, native.COMPONENT_DTYPE))
    return out


def same(got, want, labels=True, clean=True):
    """the device's outputs against the restatement's per-plane tuples: a list of what differs"""
    bad = []
    for a, (w_lab, w_clean, w_comps, w_counts) in enumerate(want):
        if labels and got["labels"][a].tobytes() != w_lab.tobytes():
            bad.append(("labels", a, int((got["labels"][a] != w_lab).sum())))
        if clean and got["clean"][a].tobytes() != w_clean.tobytes():
            bad.append(("clean", a, int((got["clean"][a] != w_clean).sum())))
        if got["counts"][a].tobytes() != w_counts.tobytes():
            bad.append(("counts", a, got["counts"][a].tolist(), w_counts.tolist()))
        if got["comps"][a].tobytes() != w_comps.tobytes():
            bad.append(("comps", a, len(got["comps"][a]), len(w_comps)))
    if not got["tail_untouched"]:
        bad.append(("records past the written ones were touched",))
    return bad


# ---- 1. byte equality ---------------------------------------------------------------------------------------------------------------------
def test_every_case_equals_the_restatement_byte_for_byte(ctx, cases, wants):
    bad, n_comps, n_px = [], 0, 0
    for c, want in zip(cases, wants):
        got = run(ctx, c)
        diff = same(got, want)
        if diff:
            bad.append((c["label"], diff))
        n_comps += sum(int(w[3][0]) for w in want)
        n_px += sum(int((w[0] != R.NONE).sum()) for w in want)
    print("%d cases, %d kept components, %d labelled pixels" % (len(cases), n_comps, n_px))
    assert not bad, bad[:10]
    assert len(cases) >= 90 and n_comps > 30000 and n_px > 300000


def test_the_cap_and_the_true_total_on_the_checkerboard(ctx, cases, wants):
    k = [c["label"] for c in cases].index(("checkerboard", 4))
    got = run(ctx, cases[k])
    assert got["counts"][0].tolist() == [16705, 0] and len(got["comps"][0]) == 4096 and got["tail_untouched"]
    assert np.array_equal(got["comps"][0]["root"], np.arange(0, 2 * 4096, 2))       # the first 4096 in root order
    k8 = [c["label"] for c in cases].index(("checkerboard", 8))
    got = run(ctx, cases[k8])
    assert got["counts"][0].tolist() == [1, 0] and got["comps"][0]["n_pixels"][0] == 16705


# ---- 2. the host form ---------------------------------------------------------------------------------------------------------------------
def test_the_host_form_gives_the_device_forms_bytes(ctx, cases, wants):
    picks = [("three planes",), ("three planes", 4), ("random", 0.45, 8, 1), ("checkerboard", 4), ("max_components", 0), ("seam blob", 1, 8), ("empty",)]
    done = 0
    for c, want in zip(cases, wants):
        if not any(c["label"][:len(p)] == p for p in picks):
            continue
        out = ctx.label_components(c["planes"], cfg_of(c), labels=True, clean=True)
        for a, (w_lab, w_clean, w_comps, w_counts) in enumerate(want):
            assert out["labels"][a].tobytes() == w_lab.tobytes() and out["clean"][a].tobytes() == w_clean.tobytes(), c["label"]
            assert out["comps"][a].tobytes() == w_comps.tobytes() and out["counts"][a].tobytes() == w_counts.tobytes(), c["label"]
        only = ctx.label_components(c["planes"], cfg_of(c), labels=False, clean=False)
        assert sorted(only) == ["comps", "counts"] and np.array_equal(only["counts"], out["counts"])
        done += 1
    assert done >= len(picks)
    # the host form leaves the caller's records beyond the written ones as they were
    c = cases[[x["label"] for x in cases].index(("seam blob", 1, 8))]
    g = cfg_of(c, max_components=5)
    recs = np.full((1, 5), 0, native.COMPONENT_DTYPE)
    recs.view(np.uint8)[:] = FILL
    counts = np.zeros((1, 2), np.uint32)
    ctx._ck(ctx._L.rr_label_components(ctx._h, c["planes"].ctypes.data, 1, C.byref(g), None, None, recs.ctypes.data, counts.ctypes.data))
    assert counts[0, 0] == 1 and (recs.view(np.uint8).reshape(-1)[REC:] == FILL).all() and recs[0, 0]["flags"] & native.COMP_SEAM


# ---- 3. what is written, and what the scratch may hold ------------------------------------------------------------------------------------
def test_optional_outputs_do_not_change_the_others(ctx, cases, wants):
    for name in (("random", 0.45, 8, 1), ("three planes", 4), ("u", 4)):
        k = [c["label"] for c in cases].index(name)
        for labels, clean in ((False, True), (True, False), (False, False)):
            got = run(ctx, cases[k], labels=labels, clean=clean)
            assert same(got, wants[k], labels, clean) == [], (name, labels, clean)
    k = [c["label"][0] for c in cases].index("max_components")
    got = run(ctx, cases[k], labels=False, clean=False)            # max_components 0 and no plane asked for: the counts alone
    assert same(got, wants[k], False, False) == [] and got["counts"][0, 0] > 0


def test_determinism_garbage_scratch_and_no_stale_state(ctx, cases, wants):
    labels = [c["label"] for c in cases]
    k = labels.index(("random", 0.6, 8, 1))
    first, second = run(ctx, cases[k]), run(ctx, cases[k])
    for key in ("labels", "clean", "counts"):
        assert first[key].tobytes() == second[key].tobytes()
    assert first["comps"][0].tobytes() == second["comps"][0].tobytes()
    noisy = run(ctx, cases[k], scratch_noise=7)
    assert same(noisy, wants[k]) == []
    # a second call with another config, and another shape, on the same scratch
    k2, k3 = labels.index(("random", 0.6, 4, 0)), labels.index(("three planes",))
    again = run(ctx, cases[k2], scratch=noisy["scratch"])
    assert same(again, wants[k2]) == []
    small = run(ctx, cases[k3], scratch=noisy["scratch"])
    assert same(small, wants[k3]) == [] and noisy["scratch"].guards_intact()


def test_a_call_on_a_second_stream(ctx, cases, wants):
    k = [c["label"] for c in cases].index(("real",))
    c = cases[k]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        out = ctx.label_components_tensors(torch.from_numpy(c["planes"]).cuda(), cfg_of(c), labels=True, clean=True, stream=s.cuda_stream)
    s.synchronize()
    w_lab, w_clean, w_comps, w_counts = wants[k][0]
    assert out["labels"].cpu().numpy().view(np.uint32)[0].tobytes() == w_lab.tobytes() and out["clean"].cpu().numpy()[0].tobytes() == w_clean.tobytes()
    assert native.Context.component_records(out["comps"], out["counts"])[0].tobytes() == w_comps.tobytes()
    assert out["scratch"].numel() == ctx.components_scratch_bytes(1, cfg_of(c))


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------------
def test_native_refusals_return_minus_three_and_write_nothing(ctx, cases):
    c = cases[[x["label"] for x in cases].index(("seam blob", 1, 8))]
    planes = c["planes"]
    n, H, W = planes.shape
    d_planes = torch.from_numpy(planes).cuda()
    good = cfg_of(c, max_components=8)
    need = ctx.components_scratch_bytes(1, good)
    B = dict(labels=Guarded(4 * H * W), clean=Guarded(H * W), comps=Guarded(8 * REC), counts=Guarded(8), scratch=Guarded(need))
    L = ctx._L

    def call(g=good, planes_ptr=d_planes.data_ptr(), n_planes=1, comps="comps", counts="counts", scratch="scratch", scratch_bytes=need, clean="clean",
             off=0, cfg_null=False):
        p = lambda k: (B[k].ptr if isinstance(k, str) else k)      # noqa: E731
        return L.rr_label_components_device(ctx._h, planes_ptr, n_planes, None if cfg_null else C.byref(g), B["labels"].ptr, p(clean),
                                            None if comps is None else p(comps) + off, p(counts), p(scratch), scratch_bytes, None)

    def cfg(**kw):
        g = cfg_of(c, max_components=8)
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    bad = [dict(planes_ptr=None), dict(counts=None), dict(scratch=None), dict(cfg_null=True), dict(n_planes=0), dict(n_planes=65536),
           dict(g=cfg(height=0)), dict(g=cfg(width=8193)), dict(g=cfg(threshold=0)), dict(g=cfg(threshold=256)), dict(g=cfg(connectivity=6)),
           dict(g=cfg(wrap_x=2)), dict(g=cfg(min_pixels=0)), dict(g=cfg(max_components=-1)), dict(g=cfg(reserved_=1)),
           dict(g=cfg(width=2, height=H * W // 2)), dict(off=8), dict(scratch=B["scratch"].ptr + 8), dict(scratch_bytes=need - 1),
           dict(comps=None), dict(g=cfg(max_components=0)), dict(clean=d_planes.data_ptr())]
    for kw in bad:
        assert call(**kw) == -3, kw
        assert len(L.rr_last_error(ctx._h)) > 10, kw
    assert L.rr_label_components_device(None, d_planes.data_ptr(), 1, C.byref(good), None, None, B["comps"].ptr, B["counts"].ptr, B["scratch"].ptr, need,
                                        None) == -1
    zero = native.RRComponentsConfig()
    assert L.rr_components_scratch_bytes(1, C.byref(zero)) == 0 and L.rr_components_scratch_bytes(0, C.byref(good)) == 0
    ctx.synchronize()
    for k, b in B.items():
        assert (b.t.cpu().numpy() == FILL).all(), k                   # nothing was written, anywhere
    assert call() == 0                                                # ... and the good call goes through
    ctx.synchronize()
    assert B["counts"].body().view(np.uint32).tolist() == [1, 0]


# ---- 5. the facades -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def box_radar():
    s = icp_ref.loop_scene()
    r = radar.RadarHIP(s["verts"], s["faces"], s["face_object_id"])
    r.loadParams(params.kaist_materials(), s["object_materials"], 0)
    r.updateDynCfg(params.kaist_preset(n_reflections=2, n_samples=icp_ref.LOOP_SAMPLES, ambient_noise=0, signal_denoising=0, n_cells=200))
    r.setBeamSamples(golden_beams(icp_ref.LOOP_SAMPLES))
    return r


def test_cluster_images_of_a_simulated_batch_stay_in_hbm(box_radar):
    r = box_radar
    r._push()
    poses = native.object_poses_array(np.stack([icp_ref.loop_pose(icp_ref.LOOP_A), icp_ref.loop_pose(icp_ref.LOOP_B)]))
    imgs = torch.empty((2, 200, radar.N_ANGLES), dtype=torch.uint8, device="cuda")
    r._ctx.simulate_batch_device(poses, imgs.data_ptr(), None)
    r._ctx.synchronize()
    out = r.clusterImages(imgs, threshold=20, min_pixels=2, max_components=512)
    assert all(isinstance(out[k], torch.Tensor) and out[k].is_cuda for k in ("labels", "comps", "counts")) and "scratch" not in out
    host = imgs.cpu().numpy()
    assert (host >= 20).sum() > 200
    ref = r.clusterImages(host, threshold=20, min_pixels=2, max_components=512)       # the host form on the downloaded images
    assert out["labels"].cpu().numpy().view(np.uint32).tobytes() == ref["labels"].tobytes()
    assert out["counts"].cpu().numpy().view(np.uint32).tobytes() == ref["counts"].tobytes() and ref["counts"][:, 0].min() >= 1
    recs = native.Context.component_records(out["comps"], out["counts"])
    for a in range(2):
        assert recs[a].tobytes() == ref["comps"][a].tobytes()
        w = R.label(host[a], 20, 8, True, 2, 512)
        assert ref["labels"][a].tobytes() == w[0].tobytes() and ref["comps"][a].tobytes() == w[2].tobytes() and ref["counts"][a].tobytes() == w[3].tobytes()


def test_segment_map_feeds_the_distance_field(box_radar):
    r = box_radar
    poses = native.object_poses_array(np.stack([icp_ref.loop_pose(p) for p in (icp_ref.LOOP_A, icp_ref.LOOP_B)]))
    clouds = r.simulatePointClouds(poses, **icp_ref.LOOP_DET)
    cfg = F.loop_field_cfg()
    _, occ = r.buildOccupancyMap(clouds, radar.RadarHIP._planar_states(poses), cfg, l_hit=3, l_free=2)
    assert (occ > 128).sum() > 50
    # the room's walls are clean in simulation: two phantoms of two cells each go where no occupied cell is within four cells
    far = np.argwhere(F.distance_field(occ, cfg, 129) >= 16)            # (the field holds squared distances in cells)
    far = far[far[:, 1] < cfg.width - 1]
    assert len(far) > 100 and abs(int(far[0][0]) - int(far[len(far) // 2][0])) > 2
    occ = occ.copy()
    for y, x in (far[0], far[len(far) // 2]):
        occ[y, x] = occ[y, x + 1] = 131
    want = R.label(occ, 129, 8, False, 3, 1 << 20)
    assert want[3][1] == 2 and want[3][0] > 0, want[3]                  # the map has segments to drop and segments to keep
    clean, recs = r.segmentMap(occ, cfg, 129, min_cells=3)
    assert clean.tobytes() == want[1].tobytes() and recs.tobytes() == want[2].tobytes()
    fld = r._ctx.distance_field(clean, cfg, 129)
    assert np.array_equal(fld, F.distance_field(want[1], cfg, 129))
    assert not np.array_equal(fld, F.distance_field(occ, cfg, 129))     # dropping the phantoms changed the field
    d_clean, d_recs = r.segmentMap(torch.from_numpy(occ).cuda(), cfg, 129, min_cells=3)
    assert d_clean.is_cuda and d_clean.cpu().numpy().tobytes() == clean.tobytes() and d_recs.tobytes() == recs.tobytes()


# ---- 6. the C++ mirror --------------------------------------------------------------------------------------------------------------------
def test_cpp_cluster_and_segment_equal_the_ctypes_path(tmp_path, ctx):
    native.build()
    exe = str(tmp_path / "components_check")
    lib_dir = os.path.join(ROOT, "radarays_ros_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "components_check.cpp"), "-o", exe, "-L", lib_dir, "-lradarays_mi355", "-Wl,-rpath," + lib_dir],
                   check=True)
    n_cells, W = 64, radar.N_ANGLES
    imgs = np.stack([R.random_plane(n_cells, W, 0.3, 11), R.random_plane(n_cells, W, 0.5, 12)])
    occ = R.random_plane(48, 70, 0.35, 13)
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.int32([2, n_cells, 128, 8, 2, 300, 70, 48, 129, 3, 4]).tobytes())
        f.write(imgs.tobytes() + occ.tobytes())
    p = subprocess.run([exe, str(inp), str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    raw = open(out, "rb").read()
    g = native.components_config(n_cells, W, 128, 8, True, 2, 300)
    a = ctx.label_components(imgs, g)
    g2 = native.components_config(48, 70, 129, 4, False, 3, 4096)
    b = ctx.label_components(occ, g2, labels=False, clean=True)
    want = a["labels"].tobytes() + a["counts"].tobytes() + b"".join(x.tobytes() for x in a["comps"]) + b["clean"].tobytes() + b["comps"][0].tobytes()
    assert raw == want and len(a["comps"][0]) > 10 and len(b["comps"][0]) > 3
