"""Object annotations on the GPU (rr_notes.hip) against the numpy restatement of their definition (tests/notes_ref.py, whose closed
forms tests/test_notes_host.py checks): synthetic label planes at the shapes where the kernels change path, the labels under
detected points, the Cartesian instance mask against the u8 resampler, the chain from poses to records on the nested-box scene of
tests/test_gpu_labels.py, two streams at once, and the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import detect_ref
import notes_ref as R
import test_labels_host as H
from radarays_ros_amd import native, params, scenes
from radarays_ros_amd.native import LABEL_NONE, NOTE_DTYPE, POINT_DTYPE

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
N_FRAMES = 3
# (n_angles, n_cells, scroll): ragged (no multiple of 4, 16 or 32: element loads, a partial occupancy word); the usual width with a tile
# that is half outside the image and a scroll that wraps inside a tile; the cell limit
SHAPES = {"37x53": (37, 53, 5), "400x64": (400, 64, 123), "64x8192": (64, 8192, 0)}
LAYOUTS = ("blobs", "comb", "unique", "beyond")
MASKS = (1, 2, 4, 7)


def conv_ctx(n_cells, n_angles, scroll=0):
    """a context with a config and no mesh"""
    c = native.Context(0)
    c.set_config(params.kaist_preset(n_cells=n_cells, scroll_image=scroll), n_angles)
    return c


def geometry(ctx):
    g = ctx._rrcfg
    return dict(scroll=g.scroll_image, theta_min=g.theta_min, theta_inc=g.theta_inc, resolution=g.resolution)


def tags(rs, shape):
    """random pass (0..3) and kind bits: every class shows"""
    return (rs.randint(0, 4, shape) << 24 | (rs.rand(*shape) < 0.3).astype(np.int64) << 28).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def planes(shape, layout):
    """-> (labels uint32 [3][n_cells][n_angles], images u8, n_objects); frame 1 is all RR_LABEL_NONE"""
    A, N, _ = SHAPES[shape]
    rs = np.random.RandomState(A + N + len(layout))
    lab = np.full((N_FRAMES, N, A), LABEL_NONE, np.uint32)
    img = rs.randint(0, 256, lab.shape).astype(np.uint8)
    img[rs.rand(*lab.shape) < 0.5] = 200                # many equal peaks: the tie rule decides
    if layout in ("blobs", "beyond"):
        n_ids, n_objects = (3, 3) if layout == "blobs" else (6, 3)
        for f in (0, 2):
            for k in range(4 * n_ids):                   # rectangles, some through column 0 / azimuth 0, with holes
                b0, a0 = rs.randint(0, N), rs.randint(0, A)
                hb, ha = rs.randint(1, max(2, N // 3)), rs.randint(1, max(2, A // 3))
                rows = np.arange(b0, min(N, b0 + hb))[:, None]
                cols = (a0 + np.arange(ha))[None, :] % A
                block = (np.uint32(k % n_ids) | tags(rs, (len(rows), ha))).astype(np.uint32)
                lab[f][rows, cols] = np.where(rs.rand(len(rows), ha) < 0.8, block, lab[f][rows, cols])
    elif layout == "comb":
        n_objects = 1
        lab[0][:, 0::2] = tags(rs, (N, len(range(0, A, 2))))
        lab[2][N // 2:, 1::2] = tags(rs, (N - N // 2, len(range(1, A, 2))))
    else:                                                # every pixel names another object: no table can hold a tile
        n_objects = N * A
        ids = np.arange(N * A, dtype=np.uint32).reshape(N, A)
        lab[0] = ids | tags(rs, (N, A))
        lab[2] = ids[::-1, ::-1] | tags(rs, (N, A))
        lab[2][rs.rand(N, A) < 0.1] = LABEL_NONE
    assert (lab[1] == LABEL_NONE).all()
    return lab, img, n_objects


def annotate_gpu(ctx, labels, imgs, n_objects, mask, stream=None, sync=True):
    """rr_annotate_labels_device on fresh device buffers: the scratch and the outputs start as garbage, the tails are guarded"""
    n = len(labels)
    d_lab = torch.from_numpy(labels.view(np.int32)).to(DEV)
    d_img = None if imgs is None else torch.from_numpy(imgs).to(DEV)
    nbytes = ctx.annotate_scratch_bytes(n, n_objects)
    d_scr = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device=DEV)
    d_notes = torch.full((n * n_objects * 80 + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    d_skip = torch.full(((n + 4) * 4,), 0x5A, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    ctx.annotate_labels_device(d_lab.data_ptr(), None if d_img is None else d_img.data_ptr(), n, n_objects, d_notes.data_ptr(), d_skip.data_ptr(),
                               d_scr.data_ptr(), nbytes, mask, stream)
    keep = (d_lab, d_img, d_scr, d_notes, d_skip)

    def result():
        h_notes, h_skip, h_scr = d_notes.cpu().numpy(), d_skip.cpu().numpy(), d_scr.cpu().numpy()
        assert (h_notes[n * n_objects * 80:] == 0x5A).all() and (h_skip[n * 4:] == 0x5A).all() and (h_scr[nbytes:] == 0xA5).all()
        return h_notes[:n * n_objects * 80].view(NOTE_DTYPE).reshape(n, n_objects), h_skip[:n * 4].view(np.uint32)
    if not sync:
        return keep, result
    ctx.synchronize(stream)
    return result()


_CTX = {}


def shape_ctx(shape):
    if shape not in _CTX:
        A, N, scroll = SHAPES[shape]
        _CTX[shape] = conv_ctx(N, A, scroll)
    return _CTX[shape]


_REFS = {}


def reference(shape, layout, mask, with_imgs):
    """the restatement's records; those of the shape several tests share are computed once (the others are large)"""
    key = (shape, layout, mask, with_imgs)
    if key in _REFS:
        return _REFS[key]
    lab, img, n_objects = planes(shape, layout)
    ref = R.annotate(lab, img if with_imgs else None, n_objects, mask, **geometry(shape_ctx(shape)))
    if shape == "400x64" and layout != "unique":
        _REFS[key] = ref
    return ref


# ---- 1. synthetic planes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", MASKS + (None,), ids=["direct", "ghost", "multipath", "all", "no_image"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_annotations_match_the_restatement(shape, layout, mask):
    ctx = shape_ctx(shape)
    lab, img, n_objects = planes(shape, layout)
    with_imgs = mask is not None
    mask = 7 if mask is None else mask
    got, skipped = annotate_gpu(ctx, lab, img if with_imgs else None, n_objects, mask)
    want, want_skipped, r_ext = reference(shape, layout, mask, with_imgs)
    assert np.array_equal(skipped, want_skipped), (skipped, want_skipped)
    R.assert_notes(got, want, r_ext)
    assert (got[1]["n_extent"] == 0).all() and (got[1]["bin_min"] == 0xFFFFFFFF).all() and np.isposinf(got[1]["x_min"]).all()      # the empty frame
    assert got["n_extent"].sum() > 0
    assert (skipped[0] > 0) == (layout == "beyond") and skipped[1] == 0
    if not with_imgs:
        assert (got["peak"] == 0).all() and (got["sum_intensity"] == 0).all()
    if layout == "comb" and mask == 7:
        A = SHAPES[shape][0]
        assert got[0, 0]["az_count"] == A - 1 or A % 2 == 1          # every other azimuth: the arc leaves out one gap of one


def test_the_host_form_returns_the_same_records():
    ctx = shape_ctx("400x64")
    lab, img, n_objects = planes("400x64", "blobs")
    got, skipped = ctx.annotate_labels(lab, img, n_objects, "direct")
    want, want_skipped, r_ext = reference("400x64", "blobs", 1, True)
    assert np.array_equal(skipped, want_skipped)
    R.assert_notes(got, want, r_ext)
    dev, _ = annotate_gpu(ctx, lab, img, n_objects, 1)
    assert dev.tobytes() == got.tobytes()                 # no reduction depends on the order: the same bytes from any call


# ---- 2. the labels under detected points ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["37x53", "400x64"])
def test_label_points_equal_numpy_indexing(shape):
    A, N, _ = SHAPES[shape]
    ctx = shape_ctx(shape)
    rs = np.random.RandomState(7)
    n = 3
    img = rs.randint(0, 256, (n, N, A)).astype(np.uint8)
    img[1] = 0                                           # a frame without a detection
    lab = rs.randint(0, 1 << 32, (n, N, A), dtype=np.uint64).astype(np.uint32)
    fac = rs.randint(0, 1 << 32, (n, N, A), dtype=np.uint64).astype(np.uint32)
    vel = rs.randn(n, N, A).astype(np.float32)
    det = dict(native.DETECT_DEFAULTS, method=1, k=5)
    d_img = torch.from_numpy(img).to(DEV)
    d_offs = torch.zeros((n, A + 1), dtype=torch.int32, device=DEV)
    ctx.detect_device(d_img.data_ptr(), n, det, None, 0, d_offs.data_ptr())
    ctx.synchronize()
    totals = d_offs.cpu().numpy().view(np.uint32)[:, -1]
    assert totals[0] == totals[2] == 5 * A and totals[1] == 0
    mp = int(totals.max()) - 17                           # below the true total: the tail of the frame is not there
    d_pts = torch.zeros((n, mp * 24), dtype=torch.uint8, device=DEV)
    ctx.detect_device(d_img.data_ptr(), n, det, d_pts.data_ptr(), mp, d_offs.data_ptr())
    d_lab, d_fac, d_vel = (torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to(DEV) for x in (lab, fac, vel))
    GUARD = 0x5A5A5A5A
    outs = [torch.full((n * mp + 16,), GUARD, dtype=torch.int32, device=DEV) for _ in range(3)]
    torch.cuda.synchronize()
    ctx.label_points_device(d_pts.data_ptr(), d_offs.data_ptr(), n, mp, d_lab.data_ptr(), outs[0].data_ptr(), d_fac.data_ptr(), outs[1].data_ptr(),
                            d_vel.data_ptr(), outs[2].data_ptr())
    ctx.synchronize()
    pts = d_pts.cpu().numpy().view(POINT_DTYPE).reshape(n, mp)
    h = [o.cpu().numpy().view(np.uint32) for o in outs]
    for f in range(n):
        m = min(int(totals[f]), mp)
        b, c = pts[f, :m]["bin"], pts[f, :m]["column"]
        for out, src in zip(h, (lab, fac, vel.view(np.uint32))):
            assert np.array_equal(out[f * mp:f * mp + m], src[f][b, c])
            assert (out[f * mp + m:(f + 1) * mp] == GUARD).all()          # nothing past the written points
    assert all((o[n * mp:] == GUARD).all() for o in h)
    # labels alone: the optional planes stay away
    only = torch.full((n * mp,), GUARD, dtype=torch.int32, device=DEV)
    ctx.label_points_device(d_pts.data_ptr(), d_offs.data_ptr(), n, mp, d_lab.data_ptr(), only.data_ptr())
    ctx.synchronize()
    assert np.array_equal(only.cpu().numpy().view(np.uint32), h[0][:n * mp])


# ---- 3. the Cartesian instance mask -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [33, 256])
@pytest.mark.parametrize("n_angles,scroll", [(37, 5), (400, 123)])
def test_cartesian_labels_equal_the_u8_nearest_resampler(n_angles, scroll, width):
    N = 96
    ctx = conv_ctx(N, n_angles, scroll)
    rs = np.random.RandomState(width + n_angles)
    u8 = rs.randint(1, 256, (2, N, n_angles)).astype(np.uint8)          # no zero: a pixel beyond range is told from a pixel that reads 0
    ps = 2.2 * N * ctx._rrcfg.resolution / width                         # the corners and a rim lie beyond the last bin
    d_u8 = torch.from_numpy(u8).to(DEV)
    d_u32 = torch.from_numpy(u8.astype(np.int32)).to(DEV)
    d_c8 = torch.zeros((2, width, width), dtype=torch.uint8, device=DEV)
    d_c32 = torch.full((2 * width * width + 16,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    ctx.polar_to_cartesian_device(d_u8.data_ptr(), 2, width, ps, d_c8.data_ptr(), False)
    ctx.polar_to_cartesian_labels_device(d_u32.data_ptr(), 2, width, ps, d_c32.data_ptr())
    ctx.synchronize()
    c8 = d_c8.cpu().numpy()
    raw = d_c32.cpu().numpy().view(np.uint32)
    assert (raw[2 * width * width:] == 0x5A5A5A5A).all()
    c32 = raw[:2 * width * width].reshape(2, width, width)
    beyond = c32 == LABEL_NONE
    assert np.array_equal(np.where(beyond, 0, c32), c8.astype(np.uint32))          # pixel for pixel; RR_LABEL_NONE against 0 beyond range
    assert np.array_equal(beyond, c8 == 0) and beyond.any() and not beyond.all()
    _, _, _, outside = detect_ref.cartesian(u8[0], width, ps, False, with_cells=True, **geometry(ctx))
    assert np.mean(beyond[0] != outside) <= 1e-3
    assert np.array_equal(ctx.polar_to_cartesian_labels(u8.astype(np.uint32), width, ps), c32)          # the host form


# ---- 4. from poses to records ---------------------------------------------------------------------------------------------------------
def scene3():
    """the nested boxes of tests/test_labels_host.py and, behind the opaque outer wall (12 m) on the -x side, a third object"""
    s = H.scene()
    v2, f2 = scenes._box_tris([-16, -1, -1], [-14, 1, 1], vbase=16)
    return {"verts": np.concatenate([s["verts"], v2]), "faces": np.concatenate([s["faces"], f2]),
            "face_object_id": np.concatenate([s["face_object_id"], np.full(12, 2, np.uint32)]), "object_materials": [2, 1, 1]}


def in_arc(note, az, n_angles):
    return (az - int(note["az_begin"])) % n_angles < int(note["az_count"])


@pytest.mark.parametrize("scroll", [0, 37])
def test_simulated_annotations_are_the_restatement_of_the_provenance_labels(native_lib, scroll):
    A = H.N_ANGLES
    s = scene3()
    cfg = H.config(n_reflections=3, record_multi_path=True, scroll_image=scroll)
    c = native_lib.Context(0)
    c.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    c.set_materials(H.materials(), s["object_materials"], 0)
    c.set_config(cfg, A)
    c.set_beam_samples(H.beams())
    assert c.n_objects == 3
    poses = np.stack(H.POSE3)
    n = len(poses)
    d_img = torch.zeros((n, cfg.n_cells, A), dtype=torch.uint8, device=DEV)
    c.simulate_batch_device(poses, d_img.data_ptr())
    c.synchronize()
    plain = d_img.cpu().numpy()
    d_lab = torch.zeros((n, cfg.n_cells, A), dtype=torch.int32, device=DEV)
    c.simulate_batch_provenance_device(poses, d_img.data_ptr(), d_lab.data_ptr())
    c.synchronize()
    lab = d_lab.cpu().numpy().view(np.uint32)
    for mask in (1, 7):
        notes, skipped, imgs = c.simulate_batch_annotations(poses, mask, want_images=True)
        assert np.array_equal(imgs, plain)                   # byte-equal to rr_simulate_batch_device
        want, want_skipped, r_ext = R.annotate(lab, plain, 3, mask, **geometry(c))
        assert np.array_equal(skipped, want_skipped) and (skipped == 0).all()
        R.assert_notes(notes, want, r_ext)
    direct = c.simulate_batch_annotations(poses, "direct")[0]
    assert c.simulate_batch_annotations(poses, "direct")[2] is None
    # pose 0 stands at the origin with yaw 0.3; azimuth a looks along yaw + a * theta_inc.  The inner box's -x wall is 5 m away at bearing pi:
    # azimuth 219, bin 100.  Through the opening the outer wall is 12 m away at bearing 0: azimuth 19, bin 240
    th = float(c._rrcfg.theta_inc)
    az_wall, az_open = int(round(((np.pi - 0.3) / th) % A)), int(round(((0.0 - 0.3) / th) % A))
    assert (az_wall, az_open) == (219, 19)
    inner, outer, hidden = direct[0]
    assert inner["n_direct"] > 0 and inner["bin_min"] <= 100 <= inner["bin_max"] and in_arc(inner, az_wall, A) and not in_arc(inner, az_open, A)
    assert outer["n_direct"] > 0 and outer["bin_min"] <= 240 <= outer["bin_max"] and in_arc(outer, az_open, A)
    assert (H.NEAR_BAND[0] <= inner["bin_min"]) and (H.FAR_BAND[0] <= outer["bin_min"])
    assert inner["peak"] > 0 and inner["bin_min"] <= inner["peak_bin"] <= inner["bin_max"] and in_arc(inner, int(inner["peak_az"]), A)
    assert inner["x_min"] < -4.5 and outer["x_max"] > 11.0          # (sensor frame: the scene's turned by the pose's yaw of 0.3)
    # the third object stands behind the opaque wall: nothing names it directly
    assert (direct[:, 2]["n_direct"] == 0).all() and (direct[:, 2]["n_extent"] == 0).all()
    # ghosts are counted whatever the mask selects
    assert direct[:, :2]["n_ghost"].sum() > 0
    c.close()


def test_radar_facade_simulate_annotations():
    from radarays_ros_amd import radar
    s = scene3()
    r = radar.RadarHIP(s["verts"], s["faces"], s["face_object_id"])
    r.loadParams(H.materials(), s["object_materials"], 0)
    r.updateDynCfg(H.config(n_reflections=2))
    r.setBeamSamples(H.beams())
    notes, skipped, imgs = r.simulate_annotations(np.stack(H.POSE3[:2]), extent=["direct", "ghost"], want_images=True)
    assert notes.shape == (2, 3) and notes.dtype == NOTE_DTYPE and skipped.shape == (2,) and imgs.shape == (2, 512, H.N_ANGLES)
    assert (notes[:, :2]["n_direct"] > 0).all() and (notes[:, 2]["n_direct"] == 0).all()
    assert np.array_equal(notes["n_extent"], notes["n_direct"] + notes["n_ghost"])


# ---- 5. two streams -----------------------------------------------------------------------------------------------------------------
def test_two_streams_annotate_two_batches_at_once():
    ctx = shape_ctx("400x64")
    jobs = []
    for layout, mask in (("blobs", 7), ("beyond", 1)):
        lab, img, n_objects = planes("400x64", layout)
        s = torch.cuda.Stream(device=DEV)
        keep, result = annotate_gpu(ctx, lab, img, n_objects, mask, s.cuda_stream, sync=False)
        jobs.append((layout, mask, s, keep, result))
    torch.cuda.synchronize()
    for layout, mask, s, keep, result in jobs:
        got, skipped = result()
        want, want_skipped, r_ext = reference("400x64", layout, mask, True)
        assert np.array_equal(skipped, want_skipped)
        R.assert_notes(got, want, r_ext)


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(native_lib):
    A, N = 16, 64
    ctx = conv_ctx(N, A)
    L, h = ctx._L, ctx._h
    n, k = 2, 3
    need = ctx.annotate_scratch_bytes(n, k)
    d = {name: torch.full((size,), 7, dtype=torch.uint8, device=DEV) for name, size in
         (("lab", n * N * A * 4), ("img", n * N * A), ("notes", n * k * 80), ("skip", n * 4), ("scr", need + 64), ("pts", n * 8 * 24),
          ("offs", n * (A + 1) * 4), ("out", n * 8 * 4), ("cart", n * 8 * 8 * 4))}
    host = {name: np.full(size, 7, np.uint8) for name, size in (("lab", n * N * A * 4), ("img", n * N * A), ("notes", n * k * 80), ("skip", n * 4),
                                                                  ("cart", n * 8 * 8 * 4))}
    torch.cuda.synchronize()
    p = lambda name: d[name].data_ptr()          # noqa: E731
    hp = lambda name: host[name].ctypes.data     # noqa: E731

    def dev(**kw):
        a = dict(lab=p("lab"), img=p("img"), n=n, k=k, mask=1, notes=p("notes"), skip=p("skip"), scr=p("scr"), nbytes=need)
        a.update(kw)
        return L.rr_annotate_labels_device(h, a["lab"], a["img"], a["n"], a["k"], a["mask"], a["notes"], a["skip"], a["scr"], a["nbytes"], None)

    def hostf(**kw):
        a = dict(lab=hp("lab"), img=hp("img"), n=n, k=k, mask=1, notes=hp("notes"), skip=hp("skip"))
        a.update(kw)
        return L.rr_annotate_labels(h, a["lab"], a["img"], a["n"], a["k"], a["mask"], a["notes"], a["skip"])

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == 7).all()) for t in d.values()) and all((x == 7).all() for x in host.values())

    shared = [dict(lab=None), dict(notes=None), dict(skip=None), dict(n=0), dict(n=65536), dict(n=-1), dict(k=0), dict(k=-1), dict(k=(1 << 24) - 1),
              dict(mask=8), dict(mask=0x80000001)]
    for kw in shared + [dict(scr=None), dict(nbytes=need - 1), dict(nbytes=0), dict(scr=p("scr") + 4), dict(notes=p("notes") + 8)]:
        assert dev(**kw) == -3, kw
        assert b"rr_annotate_labels_device" in L.rr_last_error(h), kw
    for kw in shared:
        assert hostf(**kw) == -3, kw
        assert b"rr_annotate_labels" in L.rr_last_error(h), kw
    # the label-point call
    def lp(**kw):
        a = dict(pts=p("pts"), offs=p("offs"), n=n, mp=8, lab=p("lab"), fac=None, vel=None, out=p("out"), ofac=None, ovel=None)
        a.update(kw)
        return L.rr_label_points_device(h, a["pts"], a["offs"], a["n"], a["mp"], a["lab"], a["fac"], a["vel"], a["out"], a["ofac"], a["ovel"], None)
    for kw in (dict(pts=None), dict(offs=None), dict(lab=None), dict(out=None), dict(n=0), dict(n=65536), dict(mp=-1), dict(fac=p("lab")),
               dict(ofac=p("out")), dict(vel=p("lab")), dict(ovel=p("out"))):
        assert lp(**kw) == -3, kw
        assert b"rr_label_points_device" in L.rr_last_error(h), kw
    # the Cartesian call: what the u8 call refuses, and any interpolation
    def ccfg(width=8, interpolation=0, pixel_size=0.5):
        c = native.RRCartesianConfig()
        c.width, c.interpolation, c.pixel_size = width, interpolation, pixel_size
        return c
    for c in (ccfg(width=0), ccfg(width=8193), ccfg(interpolation=1), ccfg(interpolation=2), ccfg(interpolation=-1), ccfg(pixel_size=0.0),
              ccfg(pixel_size=float("nan"))):
        assert L.rr_polar_to_cartesian_labels_device(h, p("lab"), n, C.byref(c), p("cart"), None) == -3
        assert L.rr_polar_to_cartesian_labels(h, hp("lab"), n, C.byref(c), hp("cart")) == -3
    assert L.rr_polar_to_cartesian_labels_device(h, None, n, C.byref(ccfg()), p("cart"), None) == -3
    assert L.rr_polar_to_cartesian_labels_device(h, p("lab"), n, C.byref(ccfg()), None, None) == -3
    assert L.rr_polar_to_cartesian_labels_device(h, p("lab"), 0, C.byref(ccfg()), p("cart"), None) == -3
    assert L.rr_polar_to_cartesian_labels_device(h, p("lab"), n, None, p("cart"), None) == -3
    assert untouched()
    # the simulate form: -2 without a mesh, whatever else is right
    pose = np.ascontiguousarray(H.POSE3[0], np.float32)
    assert L.rr_simulate_batch_annotations(h, pose.ctypes.data, 1, 1, hp("img"), hp("notes"), hp("skip")) == -2
    assert b"rr_set_mesh" in L.rr_last_error(h)
    for kw in (dict(n=0), dict(n=65), dict(mask=8), dict(notes=None), dict(skip=None)):
        a = dict(n=1, mask=1, notes=hp("notes"), skip=hp("skip"))
        a.update(kw)
        assert L.rr_simulate_batch_annotations(h, pose.ctypes.data, a["n"], a["mask"], hp("img"), a["notes"], a["skip"]) == -3, kw
    # without a config: -2
    bare = native_lib.Context(0)
    assert L.rr_annotate_labels_device(bare._h, p("lab"), p("img"), n, k, 1, p("notes"), p("skip"), p("scr"), need, None) == -2
    assert L.rr_label_points_device(bare._h, p("pts"), p("offs"), n, 8, p("lab"), None, None, p("out"), None, None, None) == -2
    assert L.rr_polar_to_cartesian_labels_device(bare._h, p("lab"), n, C.byref(ccfg()), p("cart"), None) == -2
    assert L.rr_simulate_batch_annotations(bare._h, pose.ctypes.data, 1, 1, hp("img"), hp("notes"), hp("skip")) == -2
    bare.close()
    # more azimuths than the packed peak key holds; more cells than a label column never get past rr_set_config
    wide = native_lib.Context(0)
    wide.set_config(params.kaist_preset(n_cells=1), 65536)
    assert L.rr_annotate_labels_device(wide._h, p("lab"), None, 1, 1, 1, p("notes"), p("skip"), p("scr"), 1 << 30, None) == -3
    assert b"n_angles" in L.rr_last_error(wide._h)
    assert L.rr_label_points_device(wide._h, p("pts"), p("offs"), 1, 8, p("lab"), None, None, p("out"), None, None, None) == -3
    with pytest.raises(native_lib.RRError, match="n_cells.*rc=-3"):
        wide.set_config(params.kaist_preset(n_cells=native_lib.LABEL_MAX_CELLS + 1), 16)
    wide.close()
    assert untouched()
    # ... and the same buffers are written by a call that is right
    assert dev() == 0
    ctx.synchronize()
    assert not bool((d["notes"] == 7).all())
    ctx.close()
