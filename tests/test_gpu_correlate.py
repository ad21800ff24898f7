"""Correlative scan matching on the GPU: rr_field_pyramid_device and rr_correlate_scan_device equal the numpy restatement
(tests/correlate_ref.py) byte for byte -- the planes, and the whole record with its per-level counts -- on every case of the shared list;
write nothing outside what they own, the scratch included; do not depend on what the scratch held; give the overflow record exactly when a
list is one candidate short; agree with rr_score_poses_device at offset 0 and with themselves on two streams; the host form, the facade and
the C++ mirror give the same bytes."""
import os
import subprocess

import numpy as np
import pytest
import torch

import correlate_ref as R
import field_ref as F
import icp_ref
from common import golden_beams
from radarays_ros_amd import native, params, radar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, FILL = 256, 0xA5
REC = native.CORR_DTYPE.itemsize
CASES = R.all_cases()


@pytest.fixture(scope="module")
def ctx():
    return native.Context(0)


@pytest.fixture(scope="module")
def wants():
    """the restatement's record of every case, computed once"""
    return [R.search_case(c) for c in CASES]


class Guarded:
    """`nbytes` bytes of HBM between two guards: FILL, seeded noise or the bytes of a host array"""

    def __init__(self, nbytes=None, noise=None, data=None):
        if data is not None:
            raw = np.frombuffer(np.ascontiguousarray(data).tobytes(), np.uint8)
            nbytes = len(raw)
        self.n = int(nbytes)
        if data is not None:
            body = raw
        elif noise is not None:
            body = np.random.default_rng(noise).integers(0, 256, self.n, dtype=np.uint8)
        else:
            body = np.full(self.n, FILL, np.uint8)
        self.t = torch.from_numpy(np.concatenate([np.full(GUARD, FILL, np.uint8), body, np.full(GUARD, FILL, np.uint8)])).cuda()
        self.ptr = self.t.data_ptr() + GUARD

    def body(self):
        return self.t[GUARD:GUARD + self.n].cpu().numpy()

    def guards_intact(self):
        h = self.t.cpu().numpy()
        return bool((h[:GUARD] == FILL).all() and (h[GUARD + self.n:] == FILL).all())


def device_pyramid(ctx, field, cfg, levels, in_place=False):
    """rr_field_pyramid_device on guarded buffers -> (the Guarded pyramid, the planes uint16 [levels + 1][H][W])"""
    cells = cfg.width * cfg.height
    src = Guarded(data=field)
    if in_place:                                              # the field sits at the head of the pyramid's buffer already
        start = np.full((levels + 1, cfg.height, cfg.width), 0xA5A5, np.uint16)
        start[0] = field
        pyr = Guarded(data=start)
        ctx.field_pyramid_device(pyr.ptr, cfg, levels, pyr.ptr)
    else:
        pyr = Guarded(2 * (levels + 1) * cells)
        ctx.field_pyramid_device(src.ptr, cfg, levels, pyr.ptr)
    ctx.synchronize()
    assert pyr.guards_intact() and src.guards_intact() and src.body().tobytes() == np.ascontiguousarray(field).tobytes()
    return pyr, pyr.body().view(np.uint16).reshape(levels + 1, cfg.height, cfg.width)


def run(ctx, c, levels=None, capacity=None, scratch_noise=1, stream=None, sync=True, pyr=None):
    """rr_correlate_scan_device on guarded buffers -> (the record, the buffers)"""
    levels = c["levels"] if levels is None else levels
    k = native.corr_config(c["half_x"], c["half_y"], levels, c["capacity"] if capacity is None else capacity)
    mp, n_rot = c["max_points"], len(c["rot"])
    if pyr is None:
        pyr, planes = device_pyramid(ctx, c["field"], c["cfg"], levels)
        assert planes.tobytes() == R.pyramid(c["field"], c["cfg"], levels).tobytes(), c["label"]
    B = dict(pyr=pyr, count=Guarded(data=np.uint32([len(c["points"])])), rot=Guarded(data=c["rot"]), rec=Guarded(REC),
             scratch=Guarded(ctx.correlate_scratch_bytes(n_rot, mp, k), noise=scratch_noise))
    if mp:
        B["points"] = Guarded(data=c["points"][:mp])
    before = {name: B[name].body().tobytes() for name in ("pyr", "count", "rot", "points") if name in B}
    ctx.correlate_scan_device(B["points"].ptr if mp else None, B["count"].ptr, mp, B["rot"].ptr, n_rot, pyr.ptr, c["cfg"], k, B["rec"].ptr,
                              B["scratch"].ptr, B["scratch"].n, stream)
    if not sync:
        return None, B
    ctx.synchronize()
    return check(B, before, c["label"]), B


def check(B, before, label):
    for name, b in B.items():
        assert b.guards_intact(), (label, name)
    for name, raw in before.items():
        assert B[name].body().tobytes() == raw, (label, name)         # the inputs are as they were
    return B["rec"].body().view(native.CORR_DTYPE)[0].copy()


def show(rec):
    return {n: rec[n].tolist() for n in rec.dtype.names}


# ---- 1. the pyramid ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(1, 1), (5, 7), (37, 29), (300, 3)])
def test_pyramid_planes_equal_the_restatement(ctx, W, H):
    rs = np.random.RandomState(100 * W + H)
    for density, md in ((0.0, 5), (0.03, 9), (0.4, 255)):
        cfg = F.grid_cfg(W, H, md)
        fld = F.distance_field((rs.random_sample((H, W)) < density).astype(np.uint8), cfg)
        levels = min(R.MAX_LEVELS, int(np.ceil(np.log2(max(W, H)))) + 1)
        want = R.pyramid(fld, cfg, levels)
        for in_place in (False, True):
            assert device_pyramid(ctx, fld, cfg, levels, in_place)[1].tobytes() == want.tobytes(), (W, H, density, in_place)
        assert np.array_equal(ctx.field_pyramid(fld, cfg, levels), want)                 # the host form


# ---- 2. every case of the shared list -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(CASES)), ids=[c["label"] for c in CASES])
def test_the_record_equals_the_restatement(ctx, wants, k):
    c = CASES[k]
    rec, _ = run(ctx, c)
    assert rec.tobytes() == wants[k].tobytes(), (c["label"], show(rec), show(wants[k]))


def test_the_record_does_not_depend_on_the_scratch(ctx, wants):
    k = [c["label"] for c in CASES].index("room L3 12x9")
    recs = [run(ctx, CASES[k], scratch_noise=noise)[0] for noise in (None, 7, 8)]
    assert all(r.tobytes() == wants[k].tobytes() for r in recs)


# ---- 3. overflow --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["wide L4", "room L3 12x9", "random 4"])
def test_a_list_one_short_overflows_and_one_at_it_does_not(ctx, wants, label):
    k = [c["label"] for c in CASES].index(label)
    c, full = CASES[k], wants[k]
    cap = int(full["kept"][1:].max())
    assert cap > 1
    at, _ = run(ctx, c, capacity=cap)
    assert at.tobytes() == full.tobytes() and at["flags"] == 0
    over, _ = run(ctx, c, capacity=cap - 1)
    want = R.search_case(c, capacity=cap - 1)
    assert over.tobytes() == want.tobytes(), (show(over), show(want))
    assert over["flags"] == native.CORR_OVERFLOW and over["sum_d2"] == over["upper"] == full["upper"]


# ---- 4. levels 0 against levels 4 ------------------------------------------------------------------------------------------------------------------
def test_the_exhaustive_and_the_pruned_search_agree_on_the_device(ctx):
    a, _ = run(ctx, R.wide_case(0))
    b, _ = run(ctx, R.wide_case(4))
    for name in ("rot", "dx", "dy", "flags", "sum_d2", "n_in", "n_hit"):
        assert a[name] == b[name], name
    assert a["evaluated"][0] == 9 * 81 * 81 and b["evaluated"].sum() < a["evaluated"][0] // 50 and a["upper"] == a["sum_d2"] <= b["upper"]


# ---- 5. offset 0 is rr_score_poses_device's score of the anchor state -----------------------------------------------------------------------------------
def test_the_anchor_score_equals_score_poses(ctx):
    for label in ("room L3 12x9", "nan point", "anchor east"):
        c = dict(CASES[[x["label"] for x in CASES].index(label)])
        pts, cnt, st, fld = Guarded(data=c["points"]), Guarded(data=np.uint32([len(c["points"])])), Guarded(data=c["rot"]), Guarded(data=c["field"])
        out = Guarded(len(c["rot"]) * native.FIELD_DTYPE.itemsize)
        ctx.score_poses_device(pts.ptr, cnt.ptr, len(c["points"]), st.ptr, len(c["rot"]), fld.ptr, c["cfg"], out.ptr)
        ctx.synchronize()
        scores = out.body().view(native.FIELD_DTYPE)
        for r in range(len(c["rot"])):
            one = dict(c, rot=c["rot"][r:r + 1], half_x=0, half_y=0, levels=0, capacity=1)
            rec, _ = run(ctx, one)
            assert (rec["sum_d2"], rec["n_in"], rec["n_hit"]) == (scores[r]["sum_d2"], scores[r]["n_in"], scores[r]["n_hit"]), (label, r)
            assert (rec["rot"], rec["dx"], rec["dy"], rec["evaluated"][0], rec["kept"][0]) == (0, 0, 0, 1, 1)


# ---- 6. two streams ---------------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_on_two_streams_give_the_same_records(ctx, wants):
    ka, kb = [[c["label"] for c in CASES].index(n) for n in ("wide L4", "room L2 12x9")]
    pyr_a, _ = device_pyramid(ctx, CASES[ka]["field"], CASES[ka]["cfg"], CASES[ka]["levels"])
    pyr_b, _ = device_pyramid(ctx, CASES[kb]["field"], CASES[kb]["cfg"], CASES[kb]["levels"])
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    pending = []
    for _ in range(2):
        pending.append((ka, run(ctx, CASES[ka], stream=s1.cuda_stream, sync=False, pyr=pyr_a)[1]))
        pending.append((kb, run(ctx, CASES[kb], stream=s2.cuda_stream, sync=False, pyr=pyr_b)[1]))
    s1.synchronize()
    s2.synchronize()
    for k, B in pending:
        assert check(B, {}, CASES[k]["label"]).tobytes() == wants[k].tobytes()


# ---- 7. refusals write nothing ---------------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing(ctx):
    c = R.room_case(2)
    g, k = c["cfg"], native.corr_config(12, 9, 2, 64)
    L, h = native.lib(), ctx._h
    import ctypes as C
    pyr, _ = device_pyramid(ctx, c["field"], g, 2)
    B = dict(points=Guarded(data=c["points"]), count=Guarded(data=np.uint32([len(c["points"])])), rot=Guarded(data=c["rot"]), rec=Guarded(REC),
             scratch=Guarded(ctx.correlate_scratch_bytes(9, len(c["points"]), k)))
    mp = len(c["points"])

    def call(points=B["points"].ptr, count=B["count"].ptr, max_points=mp, rot=B["rot"].ptr, n_rot=9, pyramid=pyr.ptr, grid=g, corr=k,
             rec=B["rec"].ptr, scratch=B["scratch"].ptr, nbytes=B["scratch"].n, handle=h):
        return L.rr_correlate_scan_device(handle, points, count, max_points, rot, n_rot, pyramid, C.byref(grid) if grid else None,
                                          C.byref(corr) if corr else None, rec, scratch, nbytes, None)

    assert call(handle=None) == -1
    reserved = native.corr_config(12, 9, 2, 64)
    reserved.reserved_[0] = 7
    bad_grid = native.field_config(g.width, g.height, g.cell, g.x0, g.y0, g.max_dist, g.gate)
    bad_grid.max_dist = 256
    for kw in (dict(points=None), dict(count=None), dict(rot=None), dict(pyramid=None), dict(rec=None), dict(scratch=None), dict(grid=None), dict(corr=None),
               dict(max_points=-1), dict(max_points=65537), dict(n_rot=0), dict(n_rot=4097), dict(rot=B["rot"].ptr + 2), dict(pyramid=pyr.ptr + 1),
               dict(rec=B["rec"].ptr + 8), dict(scratch=B["scratch"].ptr + 8), dict(nbytes=B["scratch"].n - 1), dict(corr=reserved), dict(grid=bad_grid),
               dict(corr=native.RRCorrConfig(2048, 9, 2, 64)), dict(corr=native.RRCorrConfig(12, 9, 9, 64)), dict(corr=native.RRCorrConfig(12, 9, 2, 0)),
               dict(corr=native.RRCorrConfig(2047, 2047, 2, 64), n_rot=129)):
        assert call(**kw) == -3, kw
    assert L.rr_field_pyramid_device(h, pyr.ptr, C.byref(g), 9, pyr.ptr, None) == -3
    assert L.rr_field_pyramid_device(h, None, C.byref(g), 2, pyr.ptr, None) == -3
    ctx.synchronize()
    for name in ("rec", "scratch"):
        assert (B[name].t.cpu().numpy() == FILL).all(), name              # nothing was written, anywhere
    assert call() == 0                                                    # ... and the good call goes through
    ctx.synchronize()
    assert B["rec"].body().view(native.CORR_DTYPE)[0].tobytes() == R.search_case(c, capacity=64).tobytes()


# ---- 8. the host form, the facade and the C++ mirror ---------------------------------------------------------------------------------------------------------------
def test_the_host_form_and_the_facade_give_the_same_record(ctx, wants):
    for label in ("room L3 12x9", "count 0 rot 3", "max_points 40 of 130", "nan point"):
        k = [c["label"] for c in CASES].index(label)
        c = CASES[k]
        pts = c["points"][:c["max_points"]] if label != "max_points 40 of 130" else c["points"][:40]
        rec = ctx.correlate_scan(pts, c["rot"], R.pyramid(c["field"], c["cfg"], c["levels"]), c["cfg"],
                                 native.corr_config(c["half_x"], c["half_y"], c["levels"], c["capacity"]))
        assert rec.tobytes() == wants[k].tobytes(), label
    c = R.room_case(3)
    s = icp_ref.loop_scene()
    r = radar.RadarHIP(s["verts"], s["faces"], s["face_object_id"])
    r.loadParams(params.kaist_materials(), s["object_materials"], 0)
    r.updateDynCfg(params.kaist_preset(n_reflections=2, n_samples=icp_ref.LOOP_SAMPLES, ambient_noise=0, signal_denoising=0, n_cells=200))
    r.setBeamSamples(golden_beams(icp_ref.LOOP_SAMPLES))
    k = native.corr_config(12, 9, 3, 1 << 12)
    want = R.search_case(c)
    for field_or_pyramid in (c["field"], R.pyramid(c["field"], c["cfg"], 5)):
        rec, pose = r.correlateScan(c["points"], R.ROOM_YAWS, R.ROOM_CENTRE, field_or_pyramid, c["cfg"], k)
        assert rec.tobytes() == want.tobytes()
        assert pose == (R.ROOM_CENTRE[0] + 5 * 0.25, R.ROOM_CENTRE[1] - 3 * 0.25, float(R.ROOM_YAWS[6]))
        assert np.allclose(pose, R.ROOM_TRUE, atol=1e-12)                 # the search finds the scan's pose


def test_cpp_correlate_equals_the_ctypes_path(tmp_path, ctx):
    native.build()
    exe = str(tmp_path / "correlate_check")
    lib_dir = os.path.join(ROOT, "radarays_ros_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "correlate_check.cpp"), "-o", exe, "-L", lib_dir, "-lradarays_mi355", "-Wl,-rpath," + lib_dir],
                   check=True)
    c = R.room_case(3)
    g = c["cfg"]
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.int32([len(c["points"]), len(R.ROOM_YAWS), g.width, g.height, g.max_dist, g.gate, 12, 9, 3, 4096]).tobytes())
        f.write(np.float32([g.cell, g.x0, g.y0]).tobytes() + np.float64(R.ROOM_CENTRE).tobytes() + np.float64(R.ROOM_YAWS).tobytes())
        f.write(c["points"].tobytes() + c["field"].tobytes())
    p = subprocess.run([exe, str(inp), str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    raw = open(out, "rb").read()
    rec = ctx.correlate_scan(c["points"], c["rot"], R.pyramid(c["field"], g, 3), g, native.corr_config(12, 9, 3, 4096))
    assert raw[:REC] == rec.tobytes() and rec.tobytes() == R.search_case(c).tobytes()
    assert np.frombuffer(raw[REC:], np.float64).tolist() == [R.ROOM_CENTRE[0] + 5 * 0.25, R.ROOM_CENTRE[1] - 3 * 0.25, float(R.ROOM_YAWS[6])]
