"""Place recognition on the GPU (rr_place.hip: rr_describe_images[_device], rr_simulate_batch_describe, rr_match_descriptors[_device])
against the numpy restatement of its definition (tests/place_ref.py).

Bounds.  Descriptors, index, shift, sse, n_best, xcorr, the order of the top_k and the full sse / shift matrices are integers and
compared bit for bit; so is psnr, which the host forms from an exact integer by the same f64 operations as the restatement.  ncc
within 1 ulp: its three inputs are exact integers, and sqrt and the divide are correctly rounded on both sides, but the GPU is free
to fuse nothing or something else than numpy around them (the argument of tests/test_gpu_shift.py)."""
import ctypes as C

import numpy as np
import pytest

import place_ref as R
from common import golden_beams
from radarays_ros_amd import native, params
from test_gpu_metrics import dark
from test_place_host import SIM, SIM_SHIFT, sim_database_poses, sim_query_pose

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
REC_BYTES = native.PLACE_DTYPE.itemsize
INT_FIELDS = ("index", "shift", "sse", "n_best", "xcorr")


def at_offset(a, offset):
    """the bytes of `a` at `offset` bytes past an aligned device allocation -> (the tensor that owns them, their address)"""
    buf = torch.zeros(a.size + offset + 16, dtype=torch.uint8, device=DEV)
    buf[offset:offset + a.size] = torch.from_numpy(np.ascontiguousarray(a).ravel()).to(DEV)
    return buf, buf.data_ptr() + offset


# ---- descriptors ----------------------------------------------------------------------------------------------------

DESCRIBE = [(200, 400, 0, 200, 10, 40, 2, 0), (200, 37, 3, 197, 7, 5, 2, 0), (3424, 400, 0, 3424, 20, 60, 3, 0), (200, 400, 0, 200, 10, 40, 2, 1)]


@pytest.mark.parametrize("case", DESCRIBE, ids=["200x400_10x40", "200x37_window_7x5_byte_path", "3424x400_20x60_three_images", "200x400_base_plus_1"])
def test_descriptors_match_the_restatement(case):
    n_cells, n_angles, cb, ce, R_, S_, n, offset = case
    ctx = native.Context(0)
    ctx.set_config(params.kaist_preset(n_cells=n_cells), n_angles)
    rs = np.random.RandomState(n_cells + n_angles + offset)
    imgs = np.stack([dark((n_cells, n_angles), rs) for _ in range(n)])
    imgs[-1] = rs.randint(0, 256, (n_cells, n_angles))
    want = np.stack([R.describe(im, cb, ce, R_, S_) for im in imgs])
    cfg = (R_, S_, cb, ce)
    own, ptr = at_offset(imgs, offset)
    d_desc = torch.full((n * R_ * S_ + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    ctx.describe_images_device(ptr, n, cfg, d_desc.data_ptr())
    ctx.synchronize()
    got = d_desc.cpu().numpy()
    assert np.array_equal(got[:n * R_ * S_].reshape(n, R_, S_), want), np.argwhere(got[:n * R_ * S_].reshape(n, R_, S_) != want)[:8]
    assert np.all(got[n * R_ * S_:] == 0x5A)                 # nothing past [n][R][S]
    assert np.array_equal(ctx.describe_images(imgs, cfg), want)
    assert np.array_equal(ctx.describe_images(imgs[0], {"n_rings": R_, "n_sectors": S_, "cell_begin": cb, "cell_end": ce}), want[:1])
    ctx.close()


def test_seventy_images_cross_the_staging_chunk():
    ctx = native.Context(0)
    ctx.set_config(params.kaist_preset(n_cells=64), 48)
    rs = np.random.RandomState(70)
    imgs = rs.randint(0, 256, (70, 64, 48)).astype(np.uint8)
    want = np.stack([R.describe(im, 1, 64, 9, 7) for im in imgs])
    assert np.array_equal(ctx.describe_images(imgs, (9, 7, 1, 64)), want)
    ctx.close()


# ---- matching -------------------------------------------------------------------------------------------------------

def descriptors(R_, S_, n_db, n_query, seed):
    """database: descriptors of dark()-style images plus uniform noise ones; queries: a rolled and 30 % corrupted database entry, a
    rolled exact copy of another, then noise"""
    rs = np.random.RandomState(seed)
    db = np.where(rs.rand(n_db, 1, 1) < 0.5, dark((n_db, R_, S_), rs), rs.randint(0, 256, (n_db, R_, S_))).astype(np.uint8)
    qs = []
    for k in range(n_query):
        if k == 0:
            q = np.roll(db[n_db // 2], -3, axis=1).copy()
            hit = rs.rand(R_, S_) < 0.3
            q[hit] = rs.randint(0, 256, int(hit.sum()))
        elif k == 1:
            q = np.roll(db[n_db // 3], 2, axis=1).copy()
        else:
            q = rs.randint(0, 256, (R_, S_)).astype(np.uint8)
        qs.append(q)
    return np.stack(qs), db


_WANT = {}


def expected(key, q, db, top_k):
    if key not in _WANT:
        _WANT[key] = R.match(q, db, top_k)
    return _WANT[key]


def run_device(ctx, q, db, top_k, offset=0, want_full=True):
    """queries and database at `offset` bytes past aligned allocations, the full outputs poisoned and one row longer than needed
    -> (records, sse uint32 [nq][n_db], shift uint16 [nq][n_db])"""
    nq, n = len(q), len(db)
    oq, pq = at_offset(q, offset)
    od, pd = at_offset(db, offset)
    d_sse = torch.full(((nq + 1) * n,), 0x5A5A5A5A, dtype=torch.int32, device=DEV) if want_full else None
    d_shift = torch.full(((nq + 1) * n,), 0x5A5A, dtype=torch.int16, device=DEV) if want_full else None
    torch.cuda.synchronize()
    rec = ctx.match_descriptors_device(pq, nq, pd, n, q.shape[1], q.shape[2], top_k, None if d_sse is None else d_sse.data_ptr(),
                                       None if d_shift is None else d_shift.data_ptr())
    if not want_full:
        return rec, None, None
    sse, shift = d_sse.cpu().numpy().view(np.uint32), d_shift.cpu().numpy().view(np.uint16)
    assert np.all(sse[nq * n:] == 0x5A5A5A5A) and np.all(shift[nq * n:] == 0x5A5A)          # nothing past [n_query][n_db]
    return rec, sse[:nq * n].reshape(nq, n), shift[:nq * n].reshape(nq, n)


def assert_match(rec, sse, shift, want):
    w_rec, w_sse, w_shift = want
    assert rec.shape == (len(w_rec), len(w_rec[0]))
    if sse is not None:
        assert np.array_equal(sse, w_sse), np.argwhere(sse != w_sse)[:8]
        assert np.array_equal(shift, w_shift), np.argwhere(shift != w_shift)[:8]
    for qi, row in enumerate(w_rec):
        r0, w0 = rec[qi][0], row[0]
        print("query %d: first (index %d shift %d sse %d n_best %d xcorr %d ncc %.17g psnr %r) want (%d %d %d %d %d %.17g %r)" % (
            qi, r0["index"], r0["shift"], r0["sse"], r0["n_best"], r0["xcorr"], r0["ncc"], float(r0["psnr"]),
            w0["index"], w0["shift"], w0["sse"], w0["n_best"], w0["xcorr"], w0["ncc"], w0["psnr"]))
        for k, w in enumerate(row):
            r = rec[qi][k]
            for f in INT_FIELDS:
                assert int(r[f]) == w[f], (qi, k, f, int(r[f]), w[f])
            assert float(r["psnr"]) == w["psnr"], (qi, k, float(r["psnr"]), w["psnr"])
            assert abs(r["ncc"] - w["ncc"]) <= np.spacing(abs(w["ncc"])), (qi, k, r["ncc"], w["ncc"])


SHAPES = [(20, 60, 33, 3, 5), (3, 5, 1, 1, 1), (64, 128, 40, 2, 32), (7, 9, 70001, 1, 32), (7, 9, 70001, 64, 3)]


@pytest.mark.parametrize("shape", SHAPES, ids=["20x60_db33_ragged_everything", "3x5_one_candidate", "64x128_K8192_top32", "7x9_K63_byte_path_many_slices",
                                              "7x9_64_queries_two_database_chunks"])
def test_matches_equal_the_restatement(shape):
    R_, S_, n_db, n_query, top_k = shape
    ctx = native.Context(0)                              # no config, no mesh
    q, db = descriptors(R_, S_, n_db, n_query, R_ + S_ + n_db)
    want = expected(shape, q, db, top_k)
    rec, sse, shift = run_device(ctx, q, db, top_k)
    assert_match(rec, sse, shift, want)
    if n_query > 1 and n_db > 3:
        assert rec[1][0]["index"] == n_db // 3 and rec[1][0]["sse"] == 0 and rec[1][0]["shift"] == (-2) % S_ and np.isinf(rec[1][0]["psnr"])
    # two identical calls return identical bytes; without the full outputs; the host form
    again, sse2, shift2 = run_device(ctx, q, db, top_k)
    assert rec.tobytes() == again.tobytes() and sse.tobytes() == sse2.tobytes() and shift.tobytes() == shift2.tobytes()
    bare, _, _ = run_device(ctx, q, db, top_k, want_full=False)
    assert bare.tobytes() == rec.tobytes()
    h_rec, h_sse, h_shift = ctx.match_descriptors(q, db, top_k, want_full=True)
    assert h_rec.tobytes() == rec.tobytes() and np.array_equal(h_sse, sse) and np.array_equal(h_shift, shift)
    assert ctx.match_descriptors(q, db, top_k).tobytes() == rec.tobytes()
    ctx.close()


def test_both_bases_one_byte_past_alignment():
    shape = SHAPES[0]
    R_, S_, n_db, n_query, top_k = shape
    ctx = native.Context(0)
    q, db = descriptors(R_, S_, n_db, n_query, R_ + S_ + n_db)
    rec, sse, shift = run_device(ctx, q, db, top_k, offset=1)
    assert_match(rec, sse, shift, expected(shape, q, db, top_k))
    ctx.close()


def test_host_form_merges_database_chunks():
    """300000 descriptors of 63 bytes are more than the host form stages at once: its running top-k against the restatement"""
    R_, S_, n_db, top_k = 7, 9, 300000, 32
    ctx = native.Context(0)
    rs = np.random.RandomState(9)
    db = rs.randint(0, 256, (n_db, R_, S_)).astype(np.uint8)
    q = np.roll(db[299990], 4, axis=1)[None].copy()
    db[17] = db[299990]                                  # the winner twice, in the first chunk and in the last
    want = R.match(q, db, top_k)
    rec, sse, shift = ctx.match_descriptors(q, db, top_k, want_full=True)
    assert_match(rec, sse, shift, want)
    assert [int(v) for v in rec[0]["index"][:2]] == [17, 299990] and np.all(rec[0]["sse"][:2] == 0)
    ctx.close()


def test_constant_descriptors_at_the_i32_bound():
    """all-0 against all-0 and all-255 against all-255 at K = 8192: the largest signed magnitudes; every shift ties"""
    R_, S_ = 64, 128
    K = R_ * S_
    ctx = native.Context(0)
    zero, full = np.zeros((R_, S_), np.uint8), np.full((R_, S_), 255, np.uint8)
    rec, sse, shift = run_device(ctx, np.stack([zero, full]), np.stack([zero, full, zero]), 3)
    assert np.array_equal(sse, np.array([[0, 255 * 255 * K, 0], [255 * 255 * K, 0, 255 * 255 * K]], np.uint32)) and not shift.any()
    assert [int(v) for v in rec[0]["index"]] == [0, 2, 1] and [int(v) for v in rec[1]["index"]] == [1, 0, 2]
    assert np.all(rec["n_best"] == S_) and np.all(rec["shift"] == 0) and np.all(rec["ncc"] == 0.0)
    assert rec[1][0]["xcorr"] == 255 * 255 * K and rec[1][0]["sse"] == 0 and rec[0][0]["xcorr"] == 0 and rec[0][2]["sse"] == 255 * 255 * K
    assert np.isinf(rec[0][0]["psnr"]) and rec[0][2]["psnr"] == 0.0
    assert_match(rec, sse, shift, R.match(np.stack([zero, full]), np.stack([zero, full, zero]), 3))
    ctx.close()


def test_duplicates_come_back_in_index_order():
    R_, S_ = 20, 60
    ctx = native.Context(0)
    q, db = descriptors(R_, S_, 50, 1, 5)
    db[41] = db[7] = np.roll(q[0], 11, axis=1)           # the query itself, twice
    db[30] = db[12]                                      # and one more pair of twins
    rec, sse, shift = run_device(ctx, q, db, 6)
    assert_match(rec, sse, shift, R.match(q, db, 6))
    assert [int(v) for v in rec[0]["index"][:2]] == [7, 41] and np.all(rec[0]["sse"][:2] == 0) and np.all(rec[0]["shift"][:2] == 11)
    assert np.all(rec[0]["ncc"][:2] == 1.0) and np.all(rec[0]["n_best"][:2] == 1)
    assert sse[0, 30] == sse[0, 12]
    ctx.close()


# ---- the simulated case ---------------------------------------------------------------------------------------------

def sim_ctx():
    scene = SIM["scene"]()
    ctx = native.Context(0)
    ctx.set_mesh(scene["verts"], scene["faces"], scene["face_object_id"])
    ctx.set_materials(params.kaist_materials(), scene["object_materials"], 0)
    ctx.set_config(SIM["cfg"](), 400)
    ctx.set_beam_samples(golden_beams(SIM["n_samples"]))
    return ctx


def test_simulated_scan_is_found_in_the_database():
    """tests/test_place_host.py fixes the scene, the 12 poses and the query on the CPU; here everything is rendered on the GPU"""
    ctx = sim_ctx()
    cfg = (SIM["R"], SIM["S"])
    poses = sim_database_poses()
    db = ctx.simulate_batch_describe(poses, cfg)
    assert db.shape == (12, SIM["R"], SIM["S"]) and db.any()
    d_img = torch.zeros((13, SIM["n_cells"], 400), dtype=torch.uint8, device=DEV)
    ctx.simulate_batch_device(np.concatenate([poses, sim_query_pose()[None]]), d_img.data_ptr())
    ctx.synchronize()
    imgs = d_img.cpu().numpy()
    assert np.array_equal(db, ctx.describe_images(imgs[:12], cfg))          # what describe_images makes of simulate_batch_device's images
    q = ctx.describe_images(imgs[12], cfg)
    rec = ctx.match_descriptors(q, db, 3)
    print("simulated:", [(int(r["index"]), int(r["shift"]), int(r["sse"]), int(r["n_best"]), float(r["ncc"])) for r in rec[0]])
    assert rec[0][0]["index"] == SIM["hit"] and rec[0][0]["n_best"] == 1 and rec[0][0]["shift"] == SIM_SHIFT
    assert rec[0][1]["sse"] > rec[0][0]["sse"]
    assert_match(rec, None, None, R.match(q, db, 3))
    ctx.close()


def test_python_facade_builds_a_database_and_localizes():
    from radarays_ros_amd import radar
    scene = SIM["scene"]()
    r = radar.RadarHIP(scene["verts"], scene["faces"], scene["face_object_id"])
    r.loadParams(params.kaist_materials(), scene["object_materials"], 0)
    r.updateDynCfg(SIM["cfg"]())
    r.setBeamSamples(golden_beams(SIM["n_samples"]))
    poses = sim_database_poses()
    many = np.concatenate([poses] * 6)                   # 72 poses: two chunks of the batch limit
    db = r.buildPlaceDatabase(many, (SIM["R"], SIM["S"]))
    assert db.shape == (72, SIM["R"], SIM["S"]) and np.array_equal(db[:12], db[60:])
    d_db = r.buildPlaceDatabase(many, (SIM["R"], SIM["S"]), on_device=True)
    assert np.array_equal(d_db.cpu().numpy(), db)
    real = r.simulateBatch(sim_query_pose()[None])[0]
    rec, hits = r.localize(real, db, many, 2)
    d_rec, d_hits = r.localize(real, d_db, many, 2)
    assert rec.tobytes() == d_rec.tobytes() and np.array_equal(hits, d_hits)
    assert [int(v) for v in rec["index"]] == [SIM["hit"], SIM["hit"] + 12] and np.all(rec["shift"] == SIM_SHIFT)
    # the hit's pose turned by the shift's yaw is the pose the scan was taken at
    print("localize:", hits[0], "wanted", sim_query_pose())
    assert np.allclose(hits[0], sim_query_pose(), atol=1e-6) and np.array_equal(hits[0, 4:], many[SIM["hit"], 4:])


# ---- refusals -------------------------------------------------------------------------------------------------------

def test_refusals_are_negative_with_a_message_and_write_nothing():
    ctx = native.Context(0)
    L, h = ctx._L, ctx._h
    R_, S_, n_db, nq, k = 4, 8, 10, 2, 3
    q, db = descriptors(R_, S_, n_db, nq, 3)
    d_q, d_db = torch.from_numpy(q).to(DEV), torch.from_numpy(db).to(DEV)
    d_sse = torch.full((nq, n_db), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    d_shift = torch.full((nq, n_db), 0x5A5A, dtype=torch.int16, device=DEV)
    out = np.full(nq * k * REC_BYTES, 0x5A, np.uint8)
    h_sse, h_shift = np.full((nq, n_db), 0x5A5A5A5A, np.uint32), np.full((nq, n_db), 0x5A5A, np.uint16)
    o, pq, pd, ps, pf = out.ctypes.data, d_q.data_ptr(), d_db.data_ptr(), d_sse.data_ptr(), d_shift.data_ptr()

    def refused(rc, text):
        assert rc == -3, rc
        assert text in L.rr_last_error(h), L.rr_last_error(h)
    for a in ((None, nq, pd, n_db, R_, S_, k, o), (pq, nq, None, n_db, R_, S_, k, o), (pq, nq, pd, n_db, R_, S_, k, None)):
        refused(L.rr_match_descriptors_device(h, *a, ps, pf, None), b"rr_match_descriptors_device: null buffer")
    for a, text in (((pq, 0, pd, n_db, R_, S_, k), b"n_query"), ((pq, 65, pd, n_db, R_, S_, k), b"n_query"), ((pq, nq, pd, 0, R_, S_, k), b"n_db"),
                    ((pq, nq, pd, (1 << 28) + 1, R_, S_, k), b"n_db"), ((pq, nq, pd, n_db, 0, S_, k), b"n_rings"), ((pq, nq, pd, n_db, 65, S_, k), b"n_rings"),
                    ((pq, nq, pd, n_db, R_, 3, k), b"n_sectors"), ((pq, nq, pd, n_db, R_, 129, k), b"n_sectors"), ((pq, nq, pd, n_db, 65, 128, k), b"n_rings"),
                    ((pq, nq, pd, n_db, 64, 129, k), b"n_sectors"), ((pq, nq, pd, n_db, R_, S_, 0), b"top_k"), ((pq, nq, pd, n_db, R_, S_, 33), b"top_k"),
                    ((pq, nq, pd, n_db, R_, S_, 11), b"top_k")):
        refused(L.rr_match_descriptors_device(h, *a, o, ps, pf, None), text)
    refused(L.rr_match_descriptors_device(h, pq, nq, pd, n_db, R_, S_, k, o, None, pf, None), b"shift without sse")
    hq, hd = q.ctypes.data, db.ctypes.data
    refused(L.rr_match_descriptors(h, None, nq, hd, n_db, R_, S_, k, o, None, None), b"rr_match_descriptors: null buffer")
    refused(L.rr_match_descriptors(h, hq, nq, hd, n_db, R_, S_, 11, o, h_sse.ctypes.data, h_shift.ctypes.data), b"top_k")
    refused(L.rr_match_descriptors(h, hq, nq, hd, n_db, R_, S_, k, o, None, h_shift.ctypes.data), b"shift without sse")
    # the describe calls: a context without a config is -2; with one, their own refusals
    imgs = np.zeros((2, 64, 16), np.uint8)
    d_imgs = torch.from_numpy(imgs).to(DEV)
    d_desc = torch.full((2 * 4 * 8,), 0x5A, dtype=torch.uint8, device=DEV)
    h_desc = np.full(2 * 4 * 8, 0x5A, np.uint8)
    good = native.RRPlaceConfig(0, 64, 4, 8)
    pose = np.zeros((1, 7), np.float32)
    assert L.rr_describe_images_device(h, d_imgs.data_ptr(), 2, C.byref(good), d_desc.data_ptr(), None) == -2
    assert L.rr_describe_images(h, imgs.ctypes.data, 2, C.byref(good), h_desc.ctypes.data) == -2
    assert L.rr_simulate_batch_describe(h, pose.ctypes.data, 1, C.byref(good), h_desc.ctypes.data) == -2
    assert b"rr_set_config" in L.rr_last_error(h)
    ctx.set_config(params.kaist_preset(n_cells=64), 16)
    refused(L.rr_describe_images_device(h, None, 2, C.byref(good), d_desc.data_ptr(), None), b"null buffer")
    refused(L.rr_describe_images_device(h, d_imgs.data_ptr(), 2, None, d_desc.data_ptr(), None), b"null config")
    refused(L.rr_describe_images(h, imgs.ctypes.data, 2, C.byref(good), None), b"null buffer")
    for bad, text in (((0, 64, 0, 8), b"n_rings"), ((0, 64, 4, 3), b"n_sectors"), ((0, 64, 4, 17), b"more sectors"), ((0, 65, 4, 8), b"cell window"),
                      ((-1, 64, 4, 8), b"cell window"), ((10, 10, 4, 8), b"cell window"), ((10, 13, 4, 8), b"more rings"), ((0, 64, 65, 4), b"n_rings")):
        p = native.RRPlaceConfig(*bad)
        refused(L.rr_describe_images_device(h, d_imgs.data_ptr(), 2, C.byref(p), d_desc.data_ptr(), None), text)
        refused(L.rr_describe_images(h, imgs.ctypes.data, 2, C.byref(p), h_desc.ctypes.data), text)
        refused(L.rr_simulate_batch_describe(h, pose.ctypes.data, 1, C.byref(p), h_desc.ctypes.data), text)
    for n in (0, 65):
        refused(L.rr_simulate_batch_describe(h, pose.ctypes.data, n, C.byref(good), h_desc.ctypes.data), b"n must be 1..64")
    assert L.rr_simulate_batch_describe(h, pose.ctypes.data, 1, C.byref(good), h_desc.ctypes.data) == -2      # no mesh
    torch.cuda.synchronize()
    assert np.all(out == 0x5A) and np.all(h_sse == 0x5A5A5A5A) and np.all(h_shift == 0x5A5A) and np.all(h_desc == 0x5A)
    assert bool((d_sse == 0x5A5A5A5A).all()) and bool((d_shift == 0x5A5A).all()) and bool((d_desc == 0x5A).all())
    ok = ctx.match_descriptors_device(pq, nq, pd, n_db, R_, S_, k)        # the same buffers are fine
    assert ok.tobytes() == ctx.match_descriptors(q, db, k).tobytes()
    ctx.close()
