"""The argument checks of native.Context's host forms, without a GPU and without the library: what each public method refuses, the type and the
whole text of the refusal, and which of two faults it names.  The context is a stand-in whose library raises when it is touched, so every
refusal below is one made before any call into the library, and an input that is accepted shows as the entry point it reached.  Nothing
here but the last three tests names a private helper: the rest holds for any spelling of the checks behind the public methods."""
import types

import numpy as np
import pytest

from radarays_ros_amd import native

N_CELLS, N_ANGLES = 64, 16
CAP = 65536
LIST = "points must be a list of 1..65535 one-dimensional POINT_DTYPE arrays"
COUNT = "every frame must hold the points its offsets count"
OVER = "a cloud may hold at most 65536 points"
SCAN = "the scan must be a one-dimensional POINT_DTYPE array of at most 65536 points"
FIELD = native.field_config(8, 6, 1.0, 0.0, 0.0)
OCC = native.occupancy_config(3, 2, 0, N_CELLS, N_CELLS)
BEAM = native.beam_config(0, N_CELLS, N_CELLS)
CORR = native.corr_config(1, 1, 0)
FILTER = native.filter_config()


class Reached(Exception):
    """the library was called: the name of the entry point"""


class Library:
    def __getattr__(self, name):
        raise Reached(name)


@pytest.fixture
def ctx():
    c = object.__new__(native.Context)
    c.cfg, c.n_angles = types.SimpleNamespace(n_cells=N_CELLS), N_ANGLES
    c._L = Library()                  # and no _h at all: whatever touches either raises
    assert c._polar_shape() == (N_CELLS, N_ANGLES)
    return c


def cloud(k):
    p = np.zeros(k, native.POINT_DTYPE)
    p["x"] = np.arange(k)
    return p


def offsets(*lens, dtype=np.uint32, width=N_ANGLES + 1):
    o = np.zeros((len(lens), width), dtype)
    o[:, -1] = lens
    return o


def refused(text, call, *args, **kw):
    with pytest.raises(ValueError) as e:
        call(*args, **kw)
    assert str(e.value) == text


def reaches(entry, call, *args, **kw):
    with pytest.raises(Reached) as e:
        call(*args, **kw)
    assert str(e.value) == entry


# ---- a list of clouds with its offsets: the five host forms that take one ------------------------------------------------------------
def cloud_call(ctx, name):
    """(points, offsets) -> the call of that host form with every other argument in order"""
    def table(points):
        return native.identity_sweep_table(len(points) if isinstance(points, list) else 1, N_ANGLES)
    return {
        "compensate_points": lambda p, o: ctx.compensate_points(p, o, table(p)),
        "register_points": lambda p, o: ctx.register_points(p, o, cloud(3)),
        "rasterize_points": lambda p, o: ctx.rasterize_points(p, o, FIELD),
        "occupancy_update": lambda p, o: ctx.occupancy_update(p, o, FIELD, OCC),
        "scan_profile": lambda p, o: ctx.scan_profile(p, o),
    }[name]


CLOUD_CALLS = ["compensate_points", "register_points", "rasterize_points", "occupancy_update", "scan_profile"]


@pytest.mark.parametrize("name", CLOUD_CALLS)
def test_a_list_of_clouds_and_its_offsets(ctx, name):
    call = cloud_call(ctx, name)
    refused(LIST, call, [], offsets())
    refused(LIST, call, [cloud(3), np.zeros((2, 2), native.POINT_DTYPE)], offsets(3, 4))
    refused(LIST, call, [cloud(3), np.zeros(4, np.float32)], offsets(3, 4))
    refused("offsets must be uint32 [2][17], got int32 (2, 17)", call, [cloud(3), cloud(4)], offsets(3, 4, dtype=np.int32))
    refused("offsets must be uint32 [2][17], got uint32 (2, 16)", call, [cloud(3), cloud(4)], offsets(3, 4, width=N_ANGLES))
    refused(COUNT, call, [cloud(3), cloud(4)], offsets(4, 4))                 # frame 0 holds one point fewer than its offsets count
    reaches("rr_" + name, call, cloud(5), offsets(5)[0])                     # one array for a list of one, one row of offsets
    reaches("rr_" + name, call, [cloud(3), cloud(0)], offsets(3, 0))         # ... and an empty cloud beside a full one


@pytest.mark.parametrize("name", CLOUD_CALLS)
def test_a_cloud_over_the_cap(ctx, name):
    """65,537 points: refused by the four calls whose kernels index a cloud with 16 bits and a carry, taken by compensate_points"""
    call = cloud_call(ctx, name)
    big = [cloud(3), cloud(CAP + 1)]
    if name == "compensate_points":
        reaches("rr_compensate_points", call, big, offsets(3, CAP + 1))
    else:
        refused(OVER, call, big, offsets(3, CAP + 1))
        refused(OVER, call, big, offsets(3, CAP + 1, dtype=np.int32))       # the cap is looked at before the offsets
    reaches("rr_" + name, call, [cloud(CAP)], offsets(CAP))


def test_compensate_points_names_a_bad_table_after_the_offsets_and_before_the_counts(ctx):
    short = native.identity_sweep_table(1, N_ANGLES)
    refused("offsets must be uint32 [2][17], got int32 (2, 17)", ctx.compensate_points, [cloud(3), cloud(4)], offsets(4, 4, dtype=np.int32), short)
    refused("the sweep table must have shape [2][16], got (1, 16)", ctx.compensate_points, [cloud(3), cloud(4)], offsets(4, 4), short)
    refused(LIST, ctx.compensate_points, [], offsets(), short)


@pytest.mark.parametrize("name", ["rasterize_points", "occupancy_update"])
def test_states_of_posed_clouds(ctx, name):
    call = {"rasterize_points": lambda st: ctx.rasterize_points([cloud(3), cloud(4)], offsets(3, 4), FIELD, st),
            "occupancy_update": lambda st: ctx.occupancy_update([cloud(3), cloud(4)], offsets(3, 4), FIELD, OCC, st)}[name]
    refused("states must be real numbers of shape [2][4] (c, s, tx, ty), got float64 (3, 4)", call, np.zeros((3, 4)))
    refused("states must be real numbers of shape [2][4] (c, s, tx, ty), got complex128 (2, 4)", call, np.zeros((2, 4), np.complex128))
    refused("states must be real numbers of shape [2][4] (c, s, tx, ty), got float64 (8,)", call, np.zeros(8))
    refused(COUNT, lambda st: ctx.rasterize_points([cloud(3), cloud(4)], offsets(4, 4), FIELD, st), np.zeros((3, 4)))       # the clouds come first
    reaches("rr_" + name, call, native.se2_states([0.0, 1.0]))
    reaches("rr_" + name, call, np.ones((2, 4), np.int32))


def test_register_points_target_and_init(ctx):
    two, offs = [cloud(3), cloud(4)], offsets(3, 4)
    refused("the target must be a one-dimensional POINT_DTYPE array", ctx.register_points, two, offs, np.zeros((2, 2), native.POINT_DTYPE))
    refused("the target must be a one-dimensional POINT_DTYPE array", ctx.register_points, two, offs, np.zeros(4, np.float32))
    refused(OVER, ctx.register_points, two, offs, cloud(CAP + 1))
    refused("init must be real numbers of shape [2][4] (c, s, tx, ty), got float64 (2, 3)", ctx.register_points, two, offs, cloud(3), np.zeros((2, 3)))
    refused("every initial state needs a finite, non-zero (c, s)", ctx.register_points, two, offs, cloud(3), np.zeros((2, 4)))
    # of two faults: the list before the target, the target before the cap, the cap before the offsets, the counts before init
    refused(LIST, ctx.register_points, [], offs, np.zeros(4, np.float32))
    refused("the target must be a one-dimensional POINT_DTYPE array", ctx.register_points, [cloud(CAP + 1)], offsets(CAP + 1), np.zeros(4, np.float32))
    refused(OVER, ctx.register_points, two, offsets(3, 4, dtype=np.int32), cloud(CAP + 1))
    refused(COUNT, ctx.register_points, two, offsets(4, 4), cloud(3), np.zeros((2, 3)))
    reaches("rr_register_points", ctx.register_points, two, offs, cloud(0), native.se2_states([0.0, 0.1]))
    reaches("rr_register_points", ctx.register_points, two, offs, cloud(CAP))


# ---- one scan and a batch of states ---------------------------------------------------------------------------------------------------
def too_many(n_max, dtype=np.float32):
    """n_max + 1 states that cost no memory"""
    return np.broadcast_to(dtype(0), (n_max + 1, 4))


def state_cases(call, what, n_max, entry):
    text = what + " must be real numbers of shape [n][4] (c, s, tx, ty), n in 1..%d, got %%s" % n_max
    refused(text % "float32 (5, 3)", call, np.zeros((5, 3), np.float32))
    refused(text % "float32 (0, 4)", call, np.zeros((0, 4), np.float32))
    refused(text % ("float32 (%d, 4)" % (n_max + 1)), call, too_many(n_max))
    refused(text % "float64 (8,)", call, np.zeros(8))
    refused(text % "complex64 (2, 4)", call, np.zeros((2, 4), np.complex64))
    refused(text % "bool (2, 4)", call, np.zeros((2, 4), bool))
    reaches(entry, call, np.ones((2, 4), np.int64))
    reaches(entry, call, np.ones((3, 8), np.float64)[:, ::2])


def scan_cases(call, entry):
    refused(SCAN, call, np.zeros((2, 2), native.POINT_DTYPE))
    refused(SCAN, call, cloud(CAP + 1))
    refused(SCAN, call, np.zeros(4, np.float32))
    reaches(entry, call, cloud(0))
    reaches(entry, call, cloud(CAP))


def test_score_poses(ctx):
    field = np.zeros((FIELD.height, FIELD.width), np.uint16)
    scan_cases(lambda p: ctx.score_poses(p, np.ones((2, 4), np.float32), field, FIELD), "rr_score_poses")
    state_cases(lambda st: ctx.score_poses(cloud(5), st, field, FIELD), "states", native.FIELD_MAX_HYP, "rr_score_poses")
    refused(SCAN, ctx.score_poses, cloud(CAP + 1), np.zeros((5, 3)), field, FIELD)                 # the scan before the states
    refused("field must be uint16 [6][8], got uint16 (8, 6)", ctx.score_poses, cloud(5), np.ones((2, 4)), field.T, FIELD)


def test_refine_poses(ctx):
    nearest = np.zeros((FIELD.height, FIELD.width), np.uint32)
    scan_cases(lambda p: ctx.refine_poses(p, np.ones((2, 4)), nearest, FIELD), "rr_refine_poses")
    state_cases(lambda st: ctx.refine_poses(cloud(5), st, nearest, FIELD), "init", native.FIELD_MAX_HYP, "rr_refine_poses")
    refused(SCAN, ctx.refine_poses, cloud(CAP + 1), np.zeros((5, 3)), nearest, FIELD)


def test_correlate_scan(ctx):
    pyramid = np.zeros((1, FIELD.height, FIELD.width), np.uint16)
    scan_cases(lambda p: ctx.correlate_scan(p, np.ones((2, 4), np.float32), pyramid, FIELD, CORR), "rr_correlate_scan")
    state_cases(lambda st: ctx.correlate_scan(cloud(5), st, pyramid, FIELD, CORR), "the anchor states", native.CORR_MAX_ROT, "rr_correlate_scan")
    refused(SCAN, ctx.correlate_scan, cloud(CAP + 1), np.zeros((5, 3)), pyramid, FIELD, CORR)


def test_filter_move(ctx):
    state_cases(lambda st: ctx.filter_move(st, None, None, FILTER), "states", native.FILTER_MAX_N, "rr_filter_move")
    refused("ancestors must be integers in [0, 2) of shape [n_out], n_out in 1..%d" % native.FILTER_MAX_N, ctx.filter_move, np.ones((2, 4)), [0, 2], None,
            FILTER)


def test_cast_map_and_score_beams(ctx):
    field = np.zeros((FIELD.height, FIELD.width), np.uint16)
    dirs = np.zeros((N_ANGLES, 2), np.float32)
    profile = np.zeros(N_ANGLES, np.uint16)
    bad_dirs = "dirs must be real numbers of shape [16][2] (beam_directions makes them), got float32 (17, 2)"
    state_cases(lambda st: ctx.cast_map(st, dirs, field, FIELD, BEAM), "states", native.CAST_MAX_HYP, "rr_cast_map")
    state_cases(lambda st: ctx.score_beams(profile, st, dirs, field, FIELD, BEAM), "states", native.FIELD_MAX_HYP, "rr_score_beams")
    refused(bad_dirs, ctx.cast_map, np.ones((2, 4)), np.zeros((N_ANGLES + 1, 2), np.float32), field, FIELD, BEAM)
    refused(bad_dirs, ctx.score_beams, profile, np.ones((2, 4)), np.zeros((N_ANGLES + 1, 2), np.float32), field, FIELD, BEAM)
    refused("states must be real numbers of shape [n][4] (c, s, tx, ty), n in 1..65535, got float64 (5, 3)", ctx.cast_map, np.zeros((5, 3)),
            np.zeros((N_ANGLES + 1, 2), np.float32), field, FIELD, BEAM)                           # the states before the directions
    refused("the profile must be uint16 [16], got uint16 (17,)", ctx.score_beams, np.zeros(N_ANGLES + 1, np.uint16), np.ones((2, 4)), dirs, field, FIELD,
            BEAM)


# ---- what the shapers hand on, through the private functions themselves ----------------------------------------------------------------
def test_the_cloud_shaper_returns_a_zero_padded_block_contiguous_offsets_and_the_lengths():
    rng = np.random.RandomState(5)
    pts = [cloud(3), cloud(0), cloud(7)[::-1]]
    for p in pts:
        p["bin"] = rng.randint(1, 1 << 30, len(p))
    wide = np.zeros((3, 2 * (N_ANGLES + 1)), np.uint32)
    wide[:, -2] = 3, 0, 7
    for cap in (False, True):
        buf, offs, lens = native._clouds(pts, wide[:, ::2], N_ANGLES, cap)
        assert buf.dtype == native.POINT_DTYPE and buf.shape == (3, 7) and buf.flags.c_contiguous
        assert offs.dtype == np.uint32 and offs.shape == (3, N_ANGLES + 1) and offs.flags.c_contiguous and np.array_equal(offs, wide[:, ::2])
        assert list(lens) == [3, 0, 7]
        for f, p in enumerate(pts):
            assert buf[f, :len(p)].tobytes() == np.ascontiguousarray(p).tobytes()
            assert buf[f, len(p):].tobytes() == bytes((7 - len(p)) * native.POINT_DTYPE.itemsize)
    buf, offs, lens = native._clouds(cloud(0), offsets(0)[0], N_ANGLES, True)          # one empty cloud: a block of one zero point
    assert buf.shape == (1, 1) and buf.tobytes() == bytes(native.POINT_DTYPE.itemsize) and offs.shape == (1, N_ANGLES + 1) and list(lens) == [0]
    buf, _, lens = native._clouds([cloud(CAP + 1)], offsets(CAP + 1), N_ANGLES, False)
    assert buf.shape == (1, CAP + 1) and list(lens) == [CAP + 1]


def test_the_scan_shaper_returns_the_cloud_contiguous():
    p = cloud(9)
    for lo, q in ((0, p[::2]), (1, p[::2]), (None, p[::2]), (0, p[:0]), (None, p[:0])):
        out = native._scan(q, lo, "the scan")
        assert out.dtype == native.POINT_DTYPE and out.shape == (len(q),) and out.flags.c_contiguous and out.tobytes() == np.ascontiguousarray(q).tobytes()
    refused("real_points must be a one-dimensional POINT_DTYPE array of 1..65536 points", native._scan, p[:0], 1, "real_points")
    refused("real_points must be a one-dimensional POINT_DTYPE array of 1..65536 points", native._scan, cloud(CAP + 1), 1, "real_points")
    assert len(native._scan(cloud(CAP + 1), None, "the target")) == CAP + 1


def test_the_state_shaper_returns_one_float_type_contiguous():
    src = np.arange(24, dtype=np.float64).reshape(3, 8)[:, ::2] / 7.0
    for dtype in (np.float32, np.float64):
        for kw in (dict(n_max=3), dict(n=3)):
            out = native._states(src, dtype, "states", **kw)
            assert out.dtype == dtype and out.shape == (3, 4) and out.flags.c_contiguous and np.array_equal(out, src.astype(dtype))
    assert native._states(np.ones((2, 4), np.uint8), np.float64, "init", n=2).dtype == np.float64
    assert native._icp_init(None, 2) is None
    out = native._icp_init(np.ones((2, 4), np.float32), 2)
    assert out.dtype == np.float64 and out.shape == (2, 4) and out.flags.c_contiguous
