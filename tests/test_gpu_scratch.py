"""The device forms' scratch (rr_stage.h: Scratch): one pool per stream, slot i for a call's i-th request, shared by every form.  What the
sharing could break and the tests of the single forms do not see: forms of different element types taking turns in the same slots while
these grow; a form called with and without its optional caller buffers; a slot that grows while earlier calls on its stream are still
queued; two streams at once; a host form's stage beside the scratch its device form takes on the same stream.

Every expected value is the restatement's (metrics_ref, align_ref, shift_ref, place_ref, icp_ref, surfels_ref, slice_ref), held to the bound
the form's own test module states and through that module's own assertions; the image sets are those modules' smallest."""
import numpy as np
import pytest

import dynamic_ref as D
import icp_ref as P
import slice_ref as SL
import surfels_ref as SF
import test_gpu_align as TA
import test_gpu_metrics as TM
import test_gpu_place as TP
import test_gpu_shift as TS
from radarays_ros_amd import native, params
from test_gpu_icp import source_cloud, target_cloud
from test_gpu_slice import SPLIT_BAND, SPLIT_GRID, guarded, load, payload, soup_of
from test_gpu_surfels import GATE, GUARD, N_ANGLES, dev, packed, same_as_ref, source_for, target_surfels

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
POLAR = (64, 37)                    # compare and align: test_gpu_align.py's smallest shape
SHIFT = (40, 37, 3)                 # test_gpu_shift.py's smallest
PLACE_SMALL, PLACE_LARGE = TP.SHAPES[1], TP.SHAPES[0]          # one candidate; 33 candidates of 20 x 60, 3 queries, top 5
MANY = 65                           # one more than the chunk of 64


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cycled(items, n):
    return [items[k % len(items)] for k in range(n)]


@pytest.fixture(scope="module")
def polar():
    """the image set compare and align share, with both restatements' records"""
    imgs, ref = TA.shape_set(*POLAR)
    return imgs, ref, TM.expected(imgs, ref, 7, ("scratch", POLAR)), TA.expected(imgs, ref, ("set", POLAR))


@pytest.fixture(scope="module")
def cart():
    imgs, ref, _ = TS.shape_set(*SHIFT)
    return imgs, ref, TS.expected(imgs, ref, SHIFT[2], ("set", SHIFT))


# The four synchronous forms: each helper drains the device (torch.cuda.synchronize, for its uploads) before its call, so a slot of theirs
# grows on an idle stream.  Growth and overlap with work in flight are the async cases' (3 and the second half of 4)
def compare(ctx, polar, n, stream):
    imgs, ref, want, _ = polar
    d_imgs, d_ref = up(np.stack(cycled(imgs, n))), up(ref)
    torch.cuda.synchronize()
    rec = ctx.compare_images_device(d_imgs.data_ptr(), n, d_ref.data_ptr(), TM.ALL, 7, None, stream)
    TM.assert_records(rec, None, cycled(want, n), ref.size)


def align(ctx, polar, n, stream, want_curve=False):
    imgs, ref, _, want = polar
    d_imgs, d_ref = up(np.stack(cycled(imgs, n))), up(ref)
    d_curve = torch.full((n, POLAR[1]), TA.POISON, dtype=torch.int64, device=DEV) if want_curve else None
    torch.cuda.synchronize()
    rec = ctx.align_images_device(d_imgs.data_ptr(), n, d_ref.data_ptr(), 0, None, None if d_curve is None else d_curve.data_ptr(), stream)
    TA.assert_records(rec, None if d_curve is None else d_curve.cpu().numpy(), cycled(want, n))


def shift(ctx, cart, n, stream, want_surface=False):
    imgs, ref, want = cart
    H, W, S = SHIFT
    d_imgs, d_ref = up(np.stack(cycled(imgs, n))), up(ref)
    d_xc = torch.full((n, 2 * S + 1, 2 * S + 1), TS.POISON, dtype=torch.int64, device=DEV) if want_surface else None
    torch.cuda.synchronize()
    rec = ctx.shift_images_device(d_imgs.data_ptr(), n, d_ref.data_ptr(), H, W, S, None if d_xc is None else d_xc.data_ptr(), None, stream)
    TS.assert_records(rec, None if d_xc is None else d_xc.cpu().numpy(), None, cycled(want, n))


def place(ctx, shape, stream):
    R_, S_, n_db, n_query, top_k = shape
    q, db = TP.descriptors(R_, S_, n_db, n_query, R_ + S_ + n_db)
    d_q, d_db = up(q), up(db)
    torch.cuda.synchronize()
    rec = ctx.match_descriptors_device(d_q.data_ptr(), n_query, d_db.data_ptr(), n_db, R_, S_, top_k, None, None, stream)
    TP.assert_match(rec, None, None, TP.expected(shape, q, db, top_k))


# ---- 1. forms share slots on one stream ---------------------------------------------------------------------------------------------------
def test_four_forms_take_turns_in_one_streams_slots_while_they_grow(polar, cart):
    ctx = TM.conv_ctx(*POLAR)
    s = torch.cuda.Stream(device=DEV)
    for few, many, db in ((1, MANY, PLACE_SMALL), (MANY, 1, PLACE_LARGE)):
        compare(ctx, polar, few, s.cuda_stream)
        shift(ctx, cart, many, s.cuda_stream)
        place(ctx, db, s.cuda_stream)
        align(ctx, polar, few, s.cuda_stream)
    ctx.close()


# ---- 2. optional buffers do not shift slots ---------------------------------------------------------------------------------------------
def test_a_callers_curve_or_surface_buffer_does_not_move_the_other_slots(polar, cart):
    ctx = TM.conv_ctx(*POLAR)
    s = torch.cuda.Stream(device=DEV)
    for given in (True, False, True, False):
        align(ctx, polar, 3, s.cuda_stream, want_curve=given)
        shift(ctx, cart, 3, s.cuda_stream, want_surface=given)
    ctx.close()


# ---- 3. growth under queued work ------------------------------------------------------------------------------------------------------------
def icp_ctx():
    c = native.Context(0)
    c.set_config(params.kaist_preset(n_cells=64), N_ANGLES)
    return c


def register_call(line, n_frames, seed, iterations):
    """one call of either matcher's device form: its clouds, its guarded buffers on the device (uploaded on torch's stream: the caller drains the
    device ONCE after it has made every call's, before the first is enqueued)"""
    clouds, tgt = scans(line, n_frames, seed)
    pts, offs, mp = packed(clouds)
    t = tgt if line else P.points_of(tgt)
    bufs = dict(pts=dev(pts), offs=dev(offs), tgt=dev(t), cnt=dev(np.array([len(tgt)], np.uint32)),
                rec=torch.full((n_frames * 48,), GUARD, dtype=torch.uint8, device=DEV),
                corr=torch.full((n_frames * mp * 4,), GUARD, dtype=torch.uint8, device=DEV))
    return dict(line=line, clouds=clouds, tgt=tgt, mp=mp, iterations=iterations, bufs=bufs)


def enqueue_register(ctx, call, stream):
    """the call on `stream`, nothing waited for before or after: no torch call here, a device-wide synchronise would drain `stream` too"""
    b, n_tgt = call["bufs"], len(call["tgt"])
    fn = ctx.register_surfels_device if call["line"] else ctx.register_points_device
    fn(b["pts"].data_ptr(), b["offs"].data_ptr(), len(call["clouds"]), call["mp"], b["tgt"].data_ptr(), b["cnt"].data_ptr(), n_tgt,
       b["rec"].data_ptr(), None, GATE, call["iterations"], b["corr"].data_ptr(), stream)


def registered(call):
    """what a drained call left, against the restatement"""
    clouds, b = call["clouds"], call["bufs"]
    rec = b["rec"].cpu().numpy().view(native.ICP_DTYPE)
    corr = b["corr"].cpu().numpy().view(np.uint32).reshape(len(clouds), call["mp"])
    want_rec, _, want_corr = (SF if call["line"] else P).register(clouds, call["tgt"], None, GATE, call["iterations"], None, None)
    same_as_ref(rec, corr, want_rec, want_corr)
    assert rec["n_matched"].max() > 0                                # the comparison is not of empty sums


def scans(line, n_frames, seed):
    rs = np.random.RandomState(seed)
    if line:
        tgt = target_surfels(rs, 90)
        return [source_for(rs, tgt, 40 + f % 5, yaw=0.02 + 0.001 * f) for f in range(n_frames)], tgt
    tgt = target_cloud(rs, 90)
    return [source_cloud(rs, tgt, 40 + f % 5, yaw=0.02 + 0.001 * f) for f in range(n_frames)], tgt


@pytest.mark.parametrize("line", [False, True], ids=["register_points", "register_surfels"])
def test_the_accumulator_grows_under_a_queued_call(line):
    """1 frame at 64 iterations (131 launches: still queued or running when the host comes back), then at once 33 frames on the same stream: more
    than the first call's accumulator holds, so it is freed and made anew -- with the stream drained first, or the first call would lose its sums.
    The synchronous forms above grow their slots on an idle stream (their helpers drain the device); this case and the two streams below are
    the ones that grow or overlap with work in flight"""
    ctx = icp_ctx()
    s = torch.cuda.Stream(device=DEV)
    calls = [register_call(line, 1, 501, 64), register_call(line, 33, 533, 2)]
    torch.cuda.synchronize()                                          # the uploads; from here to s.synchronize() nothing waits
    for call in calls:
        enqueue_register(ctx, call, s.cuda_stream)
    s.synchronize()
    for call in calls:
        registered(call)
    ctx.close()


_SLICE = {}


def slice_want(key, soup, obj):
    if key not in _SLICE:
        _SLICE[key] = SL.slice_mesh(soup, obj, None, SPLIT_BAND, SPLIT_GRID)
    return _SLICE[key]


def test_the_slice_scratch_grows_from_two_triangles_to_a_scene():
    ctx = native.Context(0)
    s = torch.cuda.Stream(device=DEV)
    g = native._field_cfg(SPLIT_GRID)
    cells = g.width * g.height
    two = np.float32([[[-5, -4, 0.1], [6, -3, 0.3], [1, 7, 0.5]], [[-9, 2, 0.2], [-2, 3, 0.2], [-8, 9, 0.4]]])
    scene = D.split_scene()
    maps = []
    for key, soup, obj in (("two", two, np.uint32([0, 1])), ("split", soup_of(scene), scene["face_object_id"])):
        load(ctx, soup, obj)                                          # (drains the device before the scene changes)
        d_occ, d_obj = guarded(np.zeros(cells, np.uint8)), guarded(np.full(cells, SL.OBJECT_NONE, np.uint32))
        torch.cuda.synchronize()
        ctx.slice_mesh_device(SPLIT_BAND, g, d_occ.data_ptr(), d_obj.data_ptr(), None, s.cuda_stream)
        maps.append((slice_want(key, soup, obj), d_occ, d_obj))
    s.synchronize()
    for (want, want_ids), d_occ, d_obj in maps:
        assert np.array_equal(payload(d_occ, cells).reshape(g.height, g.width), want) and want.sum() > 0
        assert np.array_equal(payload(d_obj, 4 * cells).view(np.uint32).reshape(g.height, g.width), want_ids)
    ctx.close()


# ---- 4. two streams -------------------------------------------------------------------------------------------------------------------------
def test_two_streams_keep_scratch_of_their_own(polar):
    ctx = TM.conv_ctx(*POLAR)
    a, b = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    for _ in range(3):
        compare(ctx, polar, 1, a.cuda_stream)
        compare(ctx, polar, MANY, b.cuda_stream)
    ctx.close()
    ctx = icp_ctx()
    calls = [register_call(False, 2, 602, 32), register_call(False, 5, 605, 32)]
    torch.cuda.synchronize()                                          # the uploads; from here on neither stream waits for the other
    for call, stream in zip(calls, (a, b)):
        enqueue_register(ctx, call, stream.cuda_stream)
    a.synchronize(); b.synchronize()
    for call in calls:
        registered(call)
    ctx.close()


# ---- 5. a host form over its device form ------------------------------------------------------------------------------------------------
def test_a_host_forms_stage_is_not_the_scratch_a_device_call_left(polar):
    imgs, ref, want, _ = polar
    ctx = TM.conv_ctx(*POLAR)
    compare(ctx, polar, MANY, None)                                   # leaves 64 images' histograms of scratch on the context's stream
    rec, hist = ctx.compare_images(np.stack(cycled(imgs, MANY)), ref, want_hist=True)
    TM.assert_records(rec, hist, cycled(want, MANY), ref.size)
    ctx.close()
