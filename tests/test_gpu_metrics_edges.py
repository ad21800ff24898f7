"""The image metrics (rr_metrics.hip: k_joint_hist<true|false>, k_ssim, k_metrics_finish; k_score) at their tile, strip and
alignment edges against tests/metrics_ref.py.  The cases, their inputs and the proof that each case reaches its edge and that
its inputs show every window position in the mean are in tests/test_metrics_edges_host.py.

Bounds, those of tests/test_gpu_metrics.py: the joint histogram, SSE and PSNR bit for bit, SSIM and the entropies within 1e-9
absolute.  SSIM is compared with the mean of metrics_ref.ssim_map, the brute-force per-position reference.

Both histogram shapes run: the workgroup-private LDS counts (RR_METRICS_HIST unset) and global atomics (RR_METRICS_HIST=1, read
when the context is created).  The "global" cases also run the LDS shape and ask for the same histogram and record bytes."""
import numpy as np
import pytest

import metrics_ref as M
import test_metrics_edges_host as E
from radarays_ros_amd import native, params

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
TOL = 1e-9
INFO_KEYS = ("hx", "hy", "hxy", "mi", "nmi", "voi")
PSNR_INFO = native.METRIC_PSNR | native.METRIC_INFO
CANARY, GUARD = 0xA5, 64
POISON = 0x5A5A5A5A
CASES = E.cases()
HIST_SHAPES = [None, "1"]
HIST_IDS = ["lds", "global"]


def conv_ctx(n_cells, n_angles):
    """a context with a config and no mesh"""
    c = native.Context(0)
    c.set_config(params.kaist_preset(n_cells=n_cells), n_angles)
    return c


def contexts(monkeypatch, hist_shape, n_cells, n_angles, with_lds=True):
    """[context in the asked histogram shape] and, for the global-atomics shape with `with_lds`, one in the LDS shape after it"""
    monkeypatch.delenv("RR_METRICS_HIST", raising=False)
    if hist_shape is None:
        return [conv_ctx(n_cells, n_angles)]
    lds = [conv_ctx(n_cells, n_angles)] if with_lds else []
    monkeypatch.setenv("RR_METRICS_HIST", hist_shape)
    return [conv_ctx(n_cells, n_angles)] + lds


def guarded(a, offset):
    """`a` at `offset` bytes past an aligned device allocation, GUARD canary bytes before it and at least GUARD after ->
    (allocation, address, check): check() asserts that neither the canaries nor the data have changed"""
    flat = np.ascontiguousarray(a).ravel()
    host = np.full(GUARD + offset + flat.size + GUARD + 16, CANARY, np.uint8)
    host[GUARD + offset:GUARD + offset + flat.size] = flat
    buf = torch.from_numpy(host).to(DEV)
    assert buf.data_ptr() % 16 == 0

    def check():
        assert np.array_equal(buf.cpu().numpy(), host)
    return buf, buf.data_ptr() + GUARD + offset, check


def run_device(ctx, imgs, ref, which, win=7, offsets=(0, 0), want_hist=True):
    """rr_compare_images_device and rr_score_images_device on the same pointers; the histogram buffer is poisoned and one image
    longer than needed -> (records, histograms or None, psnr, sse)"""
    n = len(imgs)
    b_imgs, p_imgs, check_imgs = guarded(imgs, offsets[0])
    b_ref, p_ref, check_ref = guarded(ref, offsets[1])
    d_hist = torch.full((n + 1, 256, 256), POISON, dtype=torch.int32, device=DEV) if want_hist else None
    torch.cuda.synchronize()
    rec = ctx.compare_images_device(p_imgs, n, p_ref, which, win, None if d_hist is None else d_hist.data_ptr())
    psnr, sse = ctx.score_images_device(p_imgs, n, p_ref, want_sse=True)
    check_imgs(); check_ref()
    hist = None
    if want_hist:
        hist = d_hist.cpu().numpy().view(np.uint32)
        assert np.all(hist[n] == POISON)
        hist = hist[:n]
    return rec, hist, psnr, sse


_WANT = {}


def expected(key, imgs, ref):
    """histogram, entropies, sse and psnr of the restatement, once per input"""
    if key not in _WANT:
        out = []
        for im in imgs:
            H = M.joint_histogram(im, ref)
            sse, psnr = M.psnr(im, ref)
            out.append(dict(M.info(H), H=H, sse=sse, psnr=psnr))
        _WANT[key] = out
    return _WANT[key]


def assert_psnr_info(rec, hist, psnr, sse, want, n_px):
    for k, w in enumerate(want):
        r = rec[k]
        print("image %d: hxy %.12f (diff %.2e) mi diff %.2e nmi diff %.2e sse %d" % (
            k, r["hxy"], abs(r["hxy"] - w["hxy"]), abs(r["mi"] - w["mi"]), abs(r["nmi"] - w["nmi"]), r["sse"]))
        assert np.array_equal(hist[k], w["H"]), (k, np.argwhere(hist[k] != w["H"])[:4])
        assert int(hist[k].sum(dtype=np.uint64)) == n_px
        for key in INFO_KEYS:
            assert abs(r[key] - w[key]) <= TOL, (k, key, r[key], w[key])
        assert int(r["sse"]) == w["sse"], k
        assert (np.isinf(r["psnr"]) and r["psnr"] > 0 and w["sse"] == 0) or abs(r["psnr"] - w["psnr"]) <= TOL, (k, r["psnr"])
    # sse and psnr: the bits of rr_score_images_device on the same pointers
    assert np.array_equal(rec["sse"], sse) and np.array_equal(rec["psnr"].view(np.uint64), psnr.view(np.uint64))


# ---- k_ssim: tile seams -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", CASES["ssim"], ids=E.case_id)
def test_ssim_at_the_tile_seams(c):
    n_cells, n_angles = E.image_shape(c)
    ctx = conv_ctx(n_cells, n_angles)
    for k, (img, ref, S) in enumerate(E.ssim_pairs((n_cells, n_angles), c.win)):
        want = float(S.mean(dtype=np.float64))
        rec, _, _, _ = run_device(ctx, np.stack([img, ref]), ref, native.METRIC_SSIM, c.win, want_hist=False)
        print("pair %d: ssim %.12f want %.12f diff %.2e" % (k, rec["ssim"][0], want, abs(rec["ssim"][0] - want)))
        assert abs(rec["ssim"][0] - want) <= TOL, (k, rec["ssim"][0], want)
        assert rec["ssim"][1] == 1.0, (k, rec["ssim"][1])
    ctx.close()


# ---- k_metrics_finish: the number of SSIM partials ------------------------------------------------------------------------

@pytest.mark.parametrize("c", CASES["finish"], ids=E.case_id)
def test_finish_sums_a_stride_of_partials_one_fewer_and_two_more(c):
    ctx = conv_ctx(c.n_cells, c.n_angles)
    for k, (img, ref, S) in zip(E.FINISH_PAIRS, E.ssim_pairs((c.n_cells, c.n_angles), c.win, E.FINISH_PAIRS)):
        want = float(S.mean(dtype=np.float64))
        rec, _, _, _ = run_device(ctx, np.stack([img, ref]), ref, native.METRIC_SSIM, c.win, want_hist=False)
        print("pair %d: ssim %.12f want %.12f diff %.2e" % (k, rec["ssim"][0], want, abs(rec["ssim"][0] - want)))
        assert abs(rec["ssim"][0] - want) <= TOL, (k, rec["ssim"][0], want)
        assert rec["ssim"][1] == 1.0, (k, rec["ssim"][1])
    ctx.close()


# ---- k_joint_hist: strips, both shapes ----------------------------------------------------------------------------------

@pytest.mark.parametrize("hist_shape", HIST_SHAPES, ids=HIST_IDS)
@pytest.mark.parametrize("c", CASES["hist"], ids=E.case_id)
def test_histogram_at_the_strip_edges(c, hist_shape, monkeypatch):
    ctxs = contexts(monkeypatch, hist_shape, c.n_cells, c.n_angles)
    for name, imgs, ref in E.hist_inputs(c.n_cells, c.n_angles):
        print(name)
        want = expected((name, c.n_cells, c.n_angles), imgs, ref)
        rec, hist, psnr, sse = run_device(ctxs[0], imgs, ref, PSNR_INFO)
        assert_psnr_info(rec, hist, psnr, sse, want, c.n_px)
        assert np.all(rec["ssim"] == 0.0)
        if name == "key1":
            assert hist[0][0, 1] == c.n_px and rec["hxy"][0] == 0.0 and rec["nmi"][0] == 1.0
        elif name == "keyFFFF":
            assert hist[0][255, 255] == c.n_px and rec["hxy"][0] == 0.0 and np.isinf(rec["psnr"][0])
        elif name == "every_bin":
            assert np.all(hist[0] == 1)
            assert abs(rec["hxy"][0] - np.log(65536.0)) <= TOL and abs(rec["mi"][0]) <= TOL
            assert abs(rec["hx"][0] - np.log(256.0)) <= TOL and abs(rec["hy"][0] - np.log(256.0)) <= TOL
        for other in ctxs[1:]:                  # the LDS shape: the same bytes
            rec2, hist2, _, _ = run_device(other, imgs, ref, PSNR_INFO)
            assert hist2.tobytes() == hist.tobytes() and rec2.tobytes() == rec.tobytes(), name
    for ctx in ctxs:
        ctx.close()


# ---- hist_walk and k_score: the alignment of both operands ---------------------------------------------------------------

@pytest.mark.parametrize("hist_shape", HIST_SHAPES, ids=HIST_IDS)
@pytest.mark.parametrize("shape", E.ALIGN_SHAPES, ids=lambda s: "%dx%d" % s)
def test_both_operands_at_byte_offsets(shape, hist_shape, monkeypatch):
    n_cells, n_angles = shape
    assert [o for s, o in CASES["align"] if s == shape] == list(E.ALIGN_OFFSETS)
    ctx = contexts(monkeypatch, hist_shape, n_cells, n_angles, with_lds=False)[0]
    imgs, ref = E.dark_set(n_cells, n_angles)
    want = expected(("dark", n_cells, n_angles), imgs, ref)
    rec0, hist0, psnr0, sse0 = run_device(ctx, imgs, ref, native.METRIC_ALL)
    assert_psnr_info(rec0, hist0, psnr0, sse0, want, n_cells * n_angles)
    for k, im in enumerate(imgs):
        assert abs(rec0["ssim"][k] - M.ssim_integer(im, ref, 7)) <= TOL, k
    assert rec0["ssim"][1] == 1.0
    for offsets in E.ALIGN_OFFSETS:
        rec, hist, psnr, sse = run_device(ctx, imgs, ref, native.METRIC_ALL, offsets=offsets)
        assert rec.tobytes() == rec0.tobytes() and hist.tobytes() == hist0.tobytes(), offsets
        assert np.array_equal(sse, rec["sse"]) and np.array_equal(psnr.view(np.uint64), rec["psnr"].view(np.uint64)), offsets
        assert np.array_equal(sse, sse0) and np.array_equal(psnr.view(np.uint64), psnr0.view(np.uint64)), offsets
    ctx.close()
