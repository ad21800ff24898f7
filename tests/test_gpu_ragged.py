"""The frame chain against the oracle at ragged beam and azimuth counts, and under every pass-0 tiling.  The cases are those of
tests/test_ragged_host.py (which proves their premises on the oracle alone): 1..65 beam samples and windows of 1..33 azimuths on either
side of one wave (16 rays), one later-pass group and one chunk of 16 segments.  Every case is rendered over its window (rr_simulate:
statistics, u8 and f32 columns) and over its whole sweep with the echo stream exported (rr_simulate_batch_provenance_device); the window
must be the same columns of the sweep, byte for byte.  Section 1 holds both to the oracle echo by echo at the default tiling, section 2
holds RR_PASS0_AZ = 1, 2, 4, 8 to the default byte for byte, section 3 the column and parameter batches, section 4 the spill columns."""
import numpy as np
import pytest

import test_ragged_host as H
import test_stream_host as S
from common import image_diff, mats_tuple
from radarays_ros_amd.native import ECHO_SRC_DTYPE, unpack_info
from test_gpu_labels import SENT, provenance
from test_gpu_labels import A as SWEEP

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MEAN_DEV_TOL = 1e-5          # tests/test_gpu_parity.py
U8_MISMATCH_TOL = 1e-3       # ... pooled over all cases here: a window of one column has too few pixels for a share of its own
# Largest relative deviation of an echo's strength from the oracle's log over all cases, whole sweeps, as measured on the MI355X
# (BASELINE.md §14).  The source is the one tests/test_gpu_labels.py states for its STRENGTH_REL_DEV: one ulp of acosf per Fresnel split
# between the GPU's libm and the host's, raised by the lobe's exponent.  The test allows four times the figure, the margin that
# constant gets; an echo paired with another wave's hit is off by orders of magnitude more.
STRENGTH_REL_DEV = 2.2005e-05
TILINGS = (1, 2, 4, 8)
ENV = ("RR_PASS0_AZ", "RR_STACK_LDS", "RR_TIGHT_GRID", "RR_TIGHT_FORCE", "RR_TRACE_CHUNK", "RR_STACKLESS")          # read at rr_create


def make_ctx(native_lib, c, az=16, spill=False, cfg=None):
    """a fresh context for one case: its buffers are sized by this case alone"""
    with pytest.MonkeyPatch.context() as mp:
        for k in ENV:
            mp.delenv(k, raising=False)          # (the suite may run under one of them)
        if az != 16:
            mp.setenv("RR_PASS0_AZ", str(az))
        if spill:
            mp.setenv("RR_STACK_LDS", "1")
        ctx = native_lib.Context(0)
    s = H.scene()
    ctx.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    ctx.set_materials(H.materials(), s["object_materials"], 0)
    ctx.set_config(H.config(c) if cfg is None else cfg, c.n_angles)
    ctx.set_beam_samples(H.beams(c))
    if c.noise:
        ctx.set_noise_offsets(H.noise_offsets(c))
    return ctx


def export(ctx, c, poses):
    """(images [n][cells][n_angles], records [n][n_angles][stride], counts [n][n_angles]) of one whole-sweep provenance call; the tail
    guard behind the records is checked, rows beyond a count keep the sentinel"""
    stride = H.stride(c)
    if c.n_angles == SWEEP:
        img, _, _, ech, cnt = provenance(ctx, poses, labels=False, faces=False, stride=stride)
        return img, ech, cnt.astype(np.int64)
    poses = np.asarray(poses, np.float32).reshape(-1, 7)
    n, na = len(poses), c.n_angles
    d_img = torch.zeros((n, H.N_CELLS, na), dtype=torch.uint8, device=DEV)
    d_ech = torch.full((n * na * stride * 16 + 64,), SENT, dtype=torch.uint8, device=DEV)
    d_cnt = torch.zeros((n, na), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    ctx.simulate_batch_provenance_device(poses, d_img.data_ptr(), None, None, d_ech.data_ptr(), stride, d_cnt.data_ptr())
    ctx.synchronize()
    raw = d_ech.cpu().numpy()
    assert (raw[n * na * stride * 16:] == SENT).all()
    return d_img.cpu().numpy(), raw[:n * na * stride * 16].view(ECHO_SRC_DTYPE).reshape(n, na, stride), d_cnt.cpu().numpy().view(np.uint32).astype(np.int64)


_RUNS = {}
KEEP = ("wave_passes", "hits", "signals", "overflow")


def run(native_lib, c, az=16):
    """one case under one tiling, computed once: the window (u8, f32, statistics of rr_simulate and of rr_get_stats) and the whole
    sweep (image, echo records, counts)"""
    if (c, az) not in _RUNS:
        ctx = make_ctx(native_lib, c, az)
        u8, f32, st = ctx.simulate(H.pose(c), c.az_begin, c.az_end, want_f32=True)
        got = ctx.stats()
        img, ech, cnt = export(ctx, c, [H.pose(c)])
        ctx.close()
        r = {"u8": u8, "f32": f32, "st": {k: st[k] for k in KEEP}, "get_stats": {k: got[k] for k in KEEP}, "img": img[0], "ech": ech[0], "cnt": cnt[0]}
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _RUNS[(c, az)] = r
    return _RUNS[(c, az)]


def where(c, log, bad):
    a, k = [int(x) for x in np.argwhere(bad)[0]]
    p = int(log["passes"][a, k])
    first = int(np.flatnonzero(log["passes"][a, :int(log["counts"][a])] == p)[0])
    return "%s azimuth %d echo %d: pass %d kind %d, echo %d of its pass; %d mismatches in %d azimuths" % (
        c, a, k, p, int(log["kinds"][a, k]), k - first, int(bad.sum()), int(bad.any(1).sum()))


def strength_deviation(r, log, m):
    g, o = r["ech"]["strength"].astype(np.float64), log["strengths"].astype(np.float64)
    nz = m & (o != 0)
    return np.where(nz, np.abs(g - o) / np.where(nz, np.abs(o), 1.0), 0.0)


# ---- 1. against the oracle at the default tiling -----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", H.CASES, ids=H.IDS)
def test_case_equals_the_oracle(native_lib, oracle, c):
    """statistics and per-azimuth echo counts exact; pass, kind, face and object equal echo by echo over the whole sweep; the cell under
    the marginal rule of tests/test_gpu_stream.py; the window's image within one LSB and 1e-5 mean f32 deviation, and equal to the
    same columns of the whole-sweep image"""
    r = run(native_lib, c)
    b, e = c.az_begin, c.az_end
    o8, o32, ost, _ = H.logged(oracle, c, True)
    log = H.logged(oracle, c, False)[3]
    print("%s: gpu %s oracle %s" % (c, r["st"], {k: ost.get(k) for k in KEEP}))
    assert r["st"]["overflow"] == 0 and r["get_stats"]["overflow"] == 0
    for k in ("wave_passes", "hits", "signals"):
        assert r["st"][k] == ost[k], (c, k, r["st"], ost)
    assert r["get_stats"]["wave_passes"] == ost["wave_passes"], (c, r["get_stats"])
    assert np.array_equal(r["cnt"], log["counts"]), (c, [(a, int(r["cnt"][a]), int(log["counts"][a])) for a in np.flatnonzero(r["cnt"] != log["counts"])[:8]])
    m = S.valid(log)
    ech = r["ech"]
    assert m.shape == ech.shape and m[b:e].any()
    obj, pas, kind = unpack_info(ech["info"])
    assert (ech["info"][m] >> np.uint32(29) == 0).all()
    for name, got, want in (("pass", pas, log["passes"]), ("kind", kind, log["kinds"]), ("face", ech["face"], log["faces"]),
                            ("object", obj, H.scene()["face_object_id"][np.where(m, log["faces"], 0)])):
        bad = m & (got != want)
        assert not bad.any(), (name, where(c, log, bad), got[bad][:4], want[bad][:4])
    sentinel = np.full(1, SENT, np.uint8).repeat(16).view(ECHO_SRC_DTYPE)[0]
    assert (ech[~m] == sentinel).all(), c                                    # nothing is written beyond a count
    d = np.where(m, ech["cell"].astype(np.int64) - log["cells"], 0)
    frac, later = log["frac"], log["passes"] > 0
    for a, k in np.argwhere(d != 0)[:20]:
        print("cell differs: azimuth %d echo %d pass %d: gpu %d oracle %d frac %.9g" % (a, k, log["passes"][a, k], ech["cell"][a, k], log["cells"][a, k], frac[a, k]))
    bad = (d != 0) & ~later
    assert not bad.any(), ("pass-0 cell", where(c, log, bad))
    allowed = later & (((d == -1) & (frac < S.DELTA)) | ((d == 1) & (frac > 1.0 - S.DELTA)))
    bad = (d != 0) & ~allowed
    assert not bad.any(), ("cell", where(c, log, bad), d[bad][:4], frac[bad][:4])
    g, o = ech["strength"], log["strengths"]
    assert np.isfinite(g[m]).all()
    bad = m & ((g == 0) != (o == 0))
    assert not bad.any(), ("zero strength", where(c, log, bad))
    # the image: the window against the oracle's window, and against the whole-sweep call of the GPU itself
    dd = image_diff(r["f32"][:, b:e], o32[:, b:e], r["u8"][:, b:e], o8[:, b:e])
    print("%s: image %s, largest relative strength deviation %.6g" % (c, dd, float(strength_deviation(r, log, m).max())))
    assert dd["u8_max"] <= 1 and dd["mean_dev"] <= MEAN_DEV_TOL, (c, dd)
    assert np.array_equal(r["u8"][:, b:e], r["img"][:, b:e]), (c, np.argwhere(r["u8"][:, b:e] != r["img"][:, b:e])[:8])
    out = np.ones(c.n_angles, bool)
    out[b:e] = False
    assert not r["u8"][:, out].any() and not r["f32"][:, out].any(), c       # rr_simulate writes the simulated columns alone
    if not c.noise:                                                          # the whole sweep is the column step of its own stream
        for a in sorted({0, b, e - 1, c.n_angles - 1}):
            _, r8 = oracle.column(oracle.make_config(H.config(c), c.n_angles), ech[a, :r["cnt"][a]]["cell"], ech[a, :r["cnt"][a]]["strength"], 0.0, a, c.n_angles)
            assert np.array_equal(r["img"][:, a], r8), (c, a)


def test_one_lsb_share_pooled_over_all_cases(native_lib, oracle):
    differ = pixels = 0
    for c in H.CASES:
        r, (o8, _, _, _) = run(native_lib, c), H.logged(oracle, c, True)
        d8 = np.abs(r["u8"][:, c.az_begin:c.az_end].astype(np.int32) - o8[:, c.az_begin:c.az_end].astype(np.int32))
        assert d8.max() <= 1, c
        differ, pixels = differ + int((d8 > 0).sum()), pixels + d8.size
    print("1-LSB mismatches over all windows: %d of %d pixels (%.3g)" % (differ, pixels, differ / pixels))
    assert pixels == H.N_CELLS * sum(H.width(c) for c in H.CASES) and differ <= U8_MISMATCH_TOL * pixels, (differ, pixels)


def test_strength_equals_the_oracle_up_to_libm(native_lib, oracle):
    worst, at, exact, total = 0.0, None, 0, 0
    for c in H.CASES:
        log = H.logged(oracle, c, False)[3]
        m = S.valid(log)
        rel = strength_deviation(run(native_lib, c), log, m)
        nz = m & (log["strengths"] != 0)
        exact, total = exact + int((rel[nz] == 0).sum()), total + int(nz.sum())
        if rel.max() > worst:
            a, k = np.unravel_index(int(rel.argmax()), rel.shape)
            worst, at = float(rel.max()), (c, int(a), int(k), int(log["passes"][a, k]))
    print("largest relative strength deviation from the oracle's log over the ragged cases: %.6g at %s (bound %.6g), %d exact of %d" % (
        worst, at, 4 * STRENGTH_REL_DEV, exact, total))
    assert total > 100000 and worst <= 4 * STRENGTH_REL_DEV, (worst, at)


# ---- 2. every tiling, byte for byte -----------------------------------------------------------------------------------------------
# every n_beam and every width, the three azimuth counts, windows at the first and at the last azimuth, the Perlin case
SUBSET = [H.CASES[k] for k in (0, 3, 5, 7, 10, 12, 15, 17, 19, 22, 24, 26, 29, 32, 34, 35, 36, 38, 39)]


def test_the_subset_holds_every_beam_count_and_every_width():
    assert len(SUBSET) >= 12 and {c.n_beam for c in SUBSET} == set(H.N_BEAMS) and {H.width(c) for c in SUBSET} == set(H.WIDTHS)
    assert {c.n_angles for c in SUBSET} == set(H.N_ANGLES) and any(c.az_begin == 0 for c in SUBSET) and any(c.az_end == c.n_angles for c in SUBSET)


def same_bytes(got, ref, what):
    if got.tobytes() != ref.tobytes():
        raise AssertionError((what, np.argwhere(got.view(np.uint8).reshape(got.shape + (-1,)) != ref.view(np.uint8).reshape(ref.shape + (-1,)))[:8]))


@pytest.mark.parametrize("az", TILINGS)
@pytest.mark.parametrize("c", SUBSET, ids=[H.IDS[H.CASES.index(c)] for c in SUBSET])
def test_tiling_does_not_show(native_lib, c, az):
    """RR_PASS0_AZ = az against the default 16: image bytes, f32 columns, statistics and every byte of every exported record"""
    ref, got = run(native_lib, c), run(native_lib, c, az)
    assert got["st"] == ref["st"] and got["get_stats"] == ref["get_stats"], (c, az, got["st"], ref["st"], got["get_stats"], ref["get_stats"])
    assert ref["get_stats"]["wave_passes"] == ref["st"]["wave_passes"] > 0
    assert np.array_equal(got["cnt"], ref["cnt"]), (c, az, np.flatnonzero(got["cnt"] != ref["cnt"])[:8])
    for k in ("u8", "f32", "img", "ech"):
        assert got[k].shape == ref[k].shape
        same_bytes(got[k], ref[k], (c, az, k))


# ---- 3. batches ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("az", [4, 16])
def test_column_batch_of_three_frames_over_a_ragged_window(native_lib, az):
    """rr_simulate_batch_columns_device: n_seg = 3 x 17 segments; every frame's block equals the frame rendered alone"""
    c = H._case(33, 37, 1, 18, 4, True, 1.1)
    assert c in H.CASES and H.width(c) == 17
    poses = np.stack([H.pose(c), H.pose(c._replace(yaw=0.3)), H.pose(c._replace(yaw=-0.12))])
    poses[1, 4:] += np.float32([0.2, 0.1, -0.05])
    ctx = make_ctx(native_lib, c, az)
    block = torch.zeros((3, 17, H.N_CELLS), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    ctx.simulate_batch_columns_device(poses, c.az_begin, c.az_end, block.data_ptr())
    ctx.synchronize()
    got = block.cpu().numpy()
    for f in range(3):
        one, _, st = ctx.simulate(poses[f], c.az_begin, c.az_end)
        assert st["overflow"] == 0 and one.any()
        assert np.array_equal(got[f].T, one[:, c.az_begin:c.az_end]), (az, f)
    ctx.close()
    assert np.array_equal(got[0].T, run(native_lib, c)["u8"][:, c.az_begin:c.az_end]) and len({got[f].tobytes() for f in range(3)}) == 3


@pytest.mark.parametrize("az", [2, 16])
def test_param_sets_in_two_beam_groups_of_five_beams(native_lib, az):
    """rr_simulate_param_sets: three sets in two beam groups (pass 0 once per group: n_groups x n_loc = 2 x 17 segments, re-mapped
    through group_frame), 5 beams, pass counts 1, 3, 2; every image equals the one-by-one render bit for bit"""
    from common import golden_beams
    c = H._case(5, 17, 14, 17, 3, False, 0.3)
    assert c in H.CASES
    other = np.ascontiguousarray(golden_beams(10)[5:])
    m0 = np.array(mats_tuple(H.materials()), np.float32)
    sets = [{"materials": m0, "beam_dirs": None, "n_reflections": 1}, {"materials": m0, "beam_dirs": other, "n_reflections": 3},
            {"materials": m0, "beam_dirs": None, "n_reflections": 2}]
    ctx, ref = make_ctx(native_lib, c, az), make_ctx(native_lib, c)
    imgs, _ = ctx.simulate_param_sets(H.pose(c), sets, len(m0))
    assert imgs.shape == (3, H.N_CELLS, c.n_angles)
    for k, st in enumerate(sets):
        ref.set_beam_samples(H.beams(c) if st["beam_dirs"] is None else st["beam_dirs"])
        ref.set_config(H.config(c, st["n_reflections"]), c.n_angles)
        one, _, stt = ref.simulate(H.pose(c))
        assert stt["overflow"] == 0 and one.any()
        assert np.array_equal(imgs[k], one), (az, k, np.argwhere(imgs[k] != one)[:8])
    assert len({imgs[k].tobytes() for k in range(3)}) == 3
    ctx.close(); ref.close()


# ---- 4. spill columns ----------------------------------------------------------------------------------------------------------------
# slots0 (ensure_frame_buffers) against the ray slots pass 0 addresses, grid.x x 16 (launch_trace; one wave of 16 rays per workgroup):
#   1 segment x 3 beams, A = 1:  tiles of 16 samples x 1 segment: 1 x ceil(3 / 16) = 1 wave -> 16 slots;  slots0 = ((1 + 1) / 2) * 32 = 32
#   17 segments x 5 beams, A = 4: tiles of 4 samples x 4 segments: ceil(17 / 4) x ceil(5 / 4) = 10 waves -> 160 slots; slots0 = (11 / 2) * 32 = 160
# later passes address (segment * row + group) * 16 + ray with row = ceil(bound / 16) <= ceil(cap / 64) * 4: 16 and 544 slots of the
# 64 and 1,088 columns the spill buffer holds for these two shapes.
@pytest.mark.parametrize("c,az", [(H._case(3, 400, 17, 18, 2, True, 0.3), 1), (H._case(5, 400, 5, 22, 3, True, 0.3, noise=2), 4)], ids=["1x3-A1", "17x5-A4"])
def test_spill_columns_of_a_ragged_tile(native_lib, c, az):
    """RR_STACK_LDS=1: every stack entry but one goes through the spill buffer, whose pass-0 columns are laid out by the tiling"""
    assert c in H.CASES
    ref = run(native_lib, c)
    ctx = make_ctx(native_lib, c, az, spill=True)
    assert ctx.bvh_info()["stack_need"] > 1          # the tree of 28 triangles does spill with one entry in LDS
    u8, f32, st = ctx.simulate(H.pose(c), c.az_begin, c.az_end, want_f32=True)
    ctx.close()
    assert {k: st[k] for k in KEEP} == ref["st"], (st, ref["st"])
    same_bytes(u8, ref["u8"], (c, az, "u8"))
    same_bytes(f32, ref["f32"], (c, az, "f32"))
