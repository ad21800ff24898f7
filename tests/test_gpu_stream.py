"""The frame chain's echo stream against the oracle's log past one scan batch.  The cases are those of tests/test_stream_host.py (which
proves their premises on the oracle alone): passes of 257..512 and of more than 512 waves, azimuths of more than 1,024 and 2,048
echoes, so that the 256-wave loops of k_trace, k_shade, k_scan and k_echo_gather and the 1,024-echo chunks of k_column all go round
more than once.  Every azimuth's exported stream (rr_simulate_batch_provenance_device) is held to the oracle's extended echo log
echo by echo -- count, pass, kind, face, object, cell, strength -- then turned into the GPU's own image column by the oracle's column
step, and compared byte for byte with itself under other launch shapes (batch position, tree builder, tight trace rows)."""
import numpy as np
import pytest

import test_stream_host as H
from radarays_ros_amd.native import ECHO_SRC_DTYPE, unpack_info
from test_gpu_labels import SENT, provenance

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

A = H.N_ANGLES
RUNS = [(case, rmp) for case in H.CASES for rmp in (False, True)]
IDS = ["%s-%s" % (case, "multipath" if rmp else "path") for case, rmp in RUNS]
# Largest relative deviation of an echo's strength from the oracle's log per case (the larger of its path and multipath runs), as
# measured on the MI355X against the oracle's log (beside the 1.0687e-05 of the 24-sample nested boxes).  The source
# is the one tests/test_gpu_labels.py states for its STRENGTH_REL_DEV: one ulp of acosf per Fresnel split between the GPU's libm and
# the host's, raised by the lobe's exponent; the worst echo of case B is one of pass 3, four splits deep.  The tests allow four times
# the figure, the margin that constant gets; a wrong echo is off by orders of magnitude more.
STRENGTH_REL_DEV = {"A": 1.96641e-05, "B": 5.73626e-05, "B2": 2.76868e-05}


def make_ctx(native_lib, case, rmp=True, builder="host"):
    c = native_lib.Context(0)
    s = H.scene(case)
    c.set_mesh(s["verts"], s["faces"], s["face_object_id"], builder=builder)
    c.set_materials(H.materials(case), s["object_materials"], 0)
    c.set_config(H.config(case, rmp), A)
    c.set_beam_samples(H.beams(case))
    return c


@pytest.fixture(scope="module")
def ctxs(native_lib):
    cs = {"A": make_ctx(native_lib, "A"), "B": make_ctx(native_lib, "B")}
    cs["B2"] = cs["B"]
    yield cs
    cs["A"].close()
    cs["B"].close()


def export(c, poses, stride):
    """(images [n][cells][A], records [n][A][stride], counts [n][A]) of one provenance call"""
    img, _, _, ech, cnt = provenance(c, poses, labels=False, faces=False, stride=stride)
    return img, ech, cnt.astype(np.int64)


_RUNS = {}


def run(ctxs, case, rmp):
    """the image, exported records [A][stride] and counts [A] of one case on the shared context, computed once"""
    if (case, rmp) not in _RUNS:
        ctxs[case].set_config(H.config(case, rmp), A)
        img, ech, cnt = export(ctxs[case], [H.pose(case)], H.STRIDE[case])
        for v in (img, ech, cnt):
            v.setflags(write=False)
        _RUNS[(case, rmp)] = (img[0], ech[0], cnt[0])
    return _RUNS[(case, rmp)]


def both(ctxs, oracle, case, rmp):
    """(GPU records [A][stride], the oracle's log cut to the stride, mask of the echoes) -- once the counts agree"""
    _, ech, cnt = run(ctxs, case, rmp)
    log = H.logged(oracle, case, rmp)[2]
    assert np.array_equal(cnt, log["counts"]), ("count", case, rmp, [(a, int(cnt[a]), int(log["counts"][a])) for a in np.flatnonzero(cnt != log["counts"])[:8]])
    s = H.STRIDE[case]
    return ech, {k: (v[:, :s] if v.ndim == 2 and v.shape[1] == H.CAP else v) for k, v in log.items()}, H.valid(log)[:, :s]


def where(log, bad):
    """the first mismatch: azimuth, position in the stream, pass, position within the pass and modulo the 256-wave batch"""
    a, k = [int(x) for x in np.argwhere(bad)[0]]
    p = int(log["passes"][a, k])
    first = int(np.flatnonzero(log["passes"][a, :int(log["counts"][a])] == p)[0])
    return "azimuth %d echo %d: pass %d kind %d, echo %d of its pass (mod 256: %d); %d mismatches in %d azimuths" % (
        a, k, p, int(log["kinds"][a, k]), k - first, (k - first) % H.BATCH, int(bad.sum()), int(bad.any(1).sum()))


# ---- 1. against the oracle's extended log ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,rmp", RUNS, ids=IDS)
def test_count_equals_the_oracle(ctxs, oracle, case, rmp):
    _, log, m = both(ctxs, oracle, case, rmp)
    assert m.sum() == log["counts"].sum() and log["counts"].max() > 3 * H.BATCH


@pytest.mark.parametrize("case,rmp", RUNS, ids=IDS)
def test_pass_and_kind_equal_the_oracle(ctxs, oracle, case, rmp):
    ech, log, m = both(ctxs, oracle, case, rmp)
    _, pas, kind = unpack_info(ech["info"])
    assert (ech["info"][m] >> np.uint32(29) == 0).all()
    bad = m & (pas != log["passes"])
    assert not bad.any(), ("pass", case, rmp, where(log, bad))
    bad = m & (kind != log["kinds"])
    assert not bad.any(), ("kind", case, rmp, where(log, bad))


@pytest.mark.parametrize("case,rmp", RUNS, ids=IDS)
def test_face_and_object_equal_the_oracle(ctxs, oracle, case, rmp):
    """an echo paired with another wave's hit names another face: this is the check that sees it"""
    ech, log, m = both(ctxs, oracle, case, rmp)
    bad = m & (ech["face"] != log["faces"])
    assert not bad.any(), ("face", case, rmp, where(log, bad), ech["face"][bad][:4], log["faces"][bad][:4])
    obj, _, _ = unpack_info(ech["info"])
    bad = m & (obj != H.scene(case)["face_object_id"][np.where(m, log["faces"], 0)])
    assert not bad.any(), ("object", case, rmp, where(log, bad))
    assert len(np.unique(log["faces"][m])) > 10 and len(np.unique(obj[m])) == 2


@pytest.mark.parametrize("case,rmp", RUNS, ids=IDS)
def test_cell_equals_the_oracle(ctxs, oracle, case, rmp):
    """pass 0: equal, no exception (both sides compute it from identical inputs).  Later passes: equal, except that an echo the oracle
    marks marginal (within H.DELTA of a bin boundary) may land in the neighbouring bin across that boundary, and in no other"""
    ech, log, m = both(ctxs, oracle, case, rmp)
    d = np.where(m, ech["cell"].astype(np.int64) - log["cells"], 0)
    frac, later = log["frac"], log["passes"] > 0
    for a, k in np.argwhere(d != 0)[:200]:
        print("cell differs: %s/%s azimuth %d echo %d pass %d kind %d: gpu %d oracle %d frac %.9g margin %.3g" % (
            case, rmp, a, k, log["passes"][a, k], log["kinds"][a, k], ech["cell"][a, k], log["cells"][a, k], frac[a, k], min(frac[a, k], 1 - frac[a, k])))
    print("cells of %s/%s: %d of %d later-pass echoes differ" % (case, rmp, int((d != 0)[later].sum()), int((m & later).sum())))
    bad = (d != 0) & ~later
    assert not bad.any(), ("pass-0 cell", case, rmp, where(log, bad))
    allowed = later & (((d == -1) & (frac < H.DELTA)) | ((d == 1) & (frac > 1.0 - H.DELTA)))
    bad = (d != 0) & ~allowed
    assert not bad.any(), ("cell", case, rmp, where(log, bad), d[bad][:4], frac[bad][:4])


@pytest.mark.parametrize("case,rmp", RUNS, ids=IDS)
def test_strength_equals_the_oracle_up_to_libm(ctxs, oracle, case, rmp):
    ech, log, m = both(ctxs, oracle, case, rmp)
    g, o = ech["strength"].astype(np.float64), log["strengths"].astype(np.float64)
    assert np.isfinite(g[m]).all()
    bad = m & ((g == 0) != (o == 0))
    assert not bad.any(), ("zero strength", case, rmp, where(log, bad))
    nz = m & (o != 0)
    rel = np.where(nz, np.abs(g - o) / np.where(nz, np.abs(o), 1.0), 0.0)
    worst = float(rel.max())
    a, k = np.unravel_index(int(rel.argmax()), rel.shape)
    bound = 4 * STRENGTH_REL_DEV[case]
    print("largest relative strength deviation of %s/%s from the oracle's log: %.6g (azimuth %d echo %d pass %d, bound %.6g), %d exact of %d" % (
        case, rmp, worst, a, k, log["passes"][a, k], bound, int((rel[nz] == 0).sum()), int(nz.sum())))
    assert worst <= bound, (case, rmp, worst, where(log, rel > bound))


# ---- 2. the image is made from this stream -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,rmp", RUNS, ids=IDS)
def test_stream_through_the_oracle_column_step_gives_the_image(ctxs, oracle, case, rmp):
    """the rule of tests/test_gpu_labels.py's test of the same name, on streams of the real chain that cross one and two chunk
    boundaries of k_column"""
    img, ech, cnt = run(ctxs, case, rmp)
    cfg = oracle.make_config(H.config(case, rmp), A)
    for a in range(A):
        e = ech[a, :cnt[a]]
        _, r8 = oracle.column(cfg, e["cell"], e["strength"], 0.0, a, A)
        assert np.array_equal(img[:, a], r8), (case, rmp, a, int(cnt[a]), np.flatnonzero(img[:, a] != r8)[:8])
    assert img.any()
    if case != "A":
        assert (cnt > H.SIG_CHUNK).any() and (not rmp or (cnt > 2 * H.SIG_CHUNK).any())


# ---- 3. the launch shape must not show (GPU against GPU, every byte of every record) ------------------------------------------------
def same_records(got, cnt, ref, ref_cnt, what):
    assert np.array_equal(cnt, ref_cnt), (what, np.flatnonzero(cnt != ref_cnt)[:8])
    if got.tobytes() != ref.tobytes():
        bad = got.view(np.uint8).reshape(got.shape + (16,)) != ref.view(np.uint8).reshape(ref.shape + (16,))
        a, k, b = [int(x) for x in np.argwhere(bad)[0]]
        raise AssertionError((what, "azimuth %d echo %d (mod 256: %d) byte %d" % (a, k, k % H.BATCH, b), got[a, k], ref[a, k], int(bad.any(2).sum())))


def test_position_in_a_batch_does_not_show(ctxs):
    _, ref, ref_cnt = run(ctxs, "B", True)
    _, ref2, ref2_cnt = run(ctxs, "B2", True)
    c, s = ctxs["B"], H.STRIDE["B"]
    c.set_config(H.config("B", True), A)
    b, b2 = H.pose("B"), H.pose("B2")
    shifted = b2.copy()
    shifted[4] += 0.5
    _, ech, cnt = export(c, [b, b2, shifted, b, b2, shifted, b2, b], s)
    for f in (0, 3, 7):
        same_records(ech[f], cnt[f], ref, ref_cnt, "frame %d of 8" % f)
    assert np.array_equal(cnt[1], ref2_cnt) and np.array_equal(cnt[6], ref2_cnt) and not np.array_equal(cnt[2], ref2_cnt)
    cut = np.arange(s)[None, :] < np.minimum(ref2_cnt, s)[:, None]          # B2's rows are longer than this stride: their first s echoes
    assert np.array_equal(ech[1][cut], ref2[:, :s][cut]) and np.array_equal(ech[6][cut], ref2[:, :s][cut])


def test_tree_builder_does_not_show(ctxs, native_lib):
    c = make_ctx(native_lib, "B", True, builder="gpu")
    for case in ("B", "B2"):
        _, ref, ref_cnt = run(ctxs, case, True)
        _, ech, cnt = export(c, [H.pose(case)], H.STRIDE[case])
        same_records(ech[0], cnt[0], ref, ref_cnt, "builder=gpu, case " + case)
    c.close()


@pytest.mark.parametrize("env", [("RR_TIGHT_GRID", "0"), ("RR_TIGHT_FORCE", "1")], ids=["full_rows", "one_group_rows"])
def test_trace_row_length_does_not_show(ctxs, native_lib, monkeypatch, env):
    refs = {case: run(ctxs, case, True) for case in ("B", "B2")}
    monkeypatch.delenv("RR_TIGHT_GRID", raising=False)
    monkeypatch.delenv("RR_TIGHT_FORCE", raising=False)
    monkeypatch.delenv("RR_STACK_LDS", raising=False)          # (the spill path keeps full rows)
    monkeypatch.setenv(*env)                                   # read at rr_create
    c = make_ctx(native_lib, "B", True)
    for case in ("B", "B2", "B"):
        _, ech, cnt = export(c, [H.pose(case)], H.STRIDE[case])
        same_records(ech[0], cnt[0], refs[case][1], refs[case][2], "%s=%s, case %s" % (env + (case,)))
    rows, _, rep = c.trace_grid()
    if env[0] == "RR_TIGHT_GRID":
        assert not rows.any() and rep == 0
    else:
        assert rows[1] == rows[2] == rows[3] == 1 and rep > 1000
    c.close()


def test_rows_tightened_by_another_pose_are_repaired_and_do_not_show(ctxs, native_lib, monkeypatch):
    """a context whose history pose B set renders B2, whose later passes are longer (tests/test_stream_host.py): the tightened rows
    overflow, the repair launch traces the rest, and the stream is the one a fresh history gives"""
    refs = {case: run(ctxs, case, True) for case in ("B", "B2")}
    for k in ("RR_TIGHT_GRID", "RR_TIGHT_FORCE", "RR_STACK_LDS"):
        monkeypatch.delenv(k, raising=False)
    c = make_ctx(native_lib, "B", True)
    for k in range(2):                                          # the first call has no history (full rows), the second has B's
        _, ech, cnt = export(c, [H.pose("B")], H.STRIDE["B"])
        same_records(ech[0], cnt[0], refs["B"][1], refs["B"][2], "call %d at B" % k)
    rows, hist, rep = c.trace_grid()
    assert rep == 0 and rows[1:4].any(), (rows[:4], hist[:4])
    _, ech, cnt = export(c, [H.pose("B2")], H.STRIDE["B2"])
    rows2, hist2, rep2 = c.trace_grid()
    assert rep2 > 0 and (hist2[:4] >= hist[:4]).all() and (hist2[:4] > hist[:4]).any(), (rows2[:4], hist[:4], hist2[:4], rep2)
    same_records(ech[0], cnt[0], refs["B2"][1], refs["B2"][2], "B2 on B's history")
    c.close()


# ---- 4. truncation --------------------------------------------------------------------------------------------------------------------
def test_a_stride_below_every_count_truncates_every_row(ctxs):
    _, ref, ref_cnt = run(ctxs, "B", True)
    assert ref_cnt.min() > 1000
    ctxs["B"].set_config(H.config("B", True), A)
    _, ech, cnt = export(ctxs["B"], [H.pose("B")], 1000)          # (provenance() itself checks the sentinel behind the buffer)
    assert np.array_equal(cnt[0], ref_cnt)
    assert ech[0].tobytes() == np.ascontiguousarray(ref[:, :1000]).tobytes()
    assert ech.dtype == ECHO_SRC_DTYPE and SENT == 0x5A
