"""The per-64-poses device loop under RadarHIP.simulatePointClouds, registerPointClouds and buildLikelihoodField: which calls of the context each
of them makes, in which order, with which frame counts and point capacities, on which stream.  The loop is host control flow; the GPU is here
because the three methods allocate device tensors.  65 poses: one full chunk and a ragged one of 1."""
import numpy as np
import pytest

import icp_ref
from common import golden_beams
from radarays_ros_amd import native, params, radar

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
N_POSES, N_CELLS, N_SAMPLES = 65, 128, 4
CFAR, KSTRONGEST = dict(method=0), dict(method=1, k=2, min_intensity=1)
# the integer arguments the recorder notes, by position; simulate_batch_device is noted with its pose count, every call with its stream
NOTED = {"simulate_batch_device": (), "detect_device": (1, 4), "compensate_points_device": (2, 3), "register_points_device": (2, 3, 6, 10),
         "rasterize_points_device": (2, 3), "distance_field_device": (3,), "synchronize": ()}


@pytest.fixture(scope="module")
def sim():
    s = icp_ref.loop_scene()
    r = radar.RadarHIP(s["verts"], s["faces"], s["face_object_id"])
    r.loadParams(params.kaist_materials(), s["object_materials"], 0)
    r.updateDynCfg(params.kaist_preset(n_reflections=1, n_samples=N_SAMPLES, ambient_noise=0, signal_denoising=0, n_cells=N_CELLS))
    r.setBeamSamples(golden_beams(N_SAMPLES))
    return r


@pytest.fixture(scope="module")
def poses():
    """65 poses about the middle of the room, no two alike, so that the frames' totals differ"""
    return np.stack([icp_ref.loop_pose((0.02 * i, -0.01 * i, 0.003 * i)) for i in range(N_POSES)])


@pytest.fixture(scope="module")
def clouds(sim, poses):
    """what CA-CFAR finds in every frame, computed once: the clouds' lengths are the totals the loop sizes its buffers by"""
    out = sim.simulatePointClouds(poses, **CFAR)
    assert len(out) == N_POSES and max(len(c) for c in out[:64]) > 1 and len(out[64]) > 1
    return out


@pytest.fixture
def calls(sim):
    """the context's device calls wrapped by a recorder that notes (name, integer arguments) and the stream, then calls through"""
    ctx, noted, streams = sim.context, [], []
    for name, at in NOTED.items():
        def through(*args, _name=name, _at=at, _inner=getattr(ctx, name)):
            noted.append((_name,) + ((len(args[0]),) if _name == "simulate_batch_device" else tuple(int(args[i]) for i in _at)))
            streams.append(args[-1])
            return _inner(*args)
        setattr(ctx, name, through)
    yield noted, streams
    for name in NOTED:
        delattr(ctx, name)


def chunks(clouds, capped):
    """(n, max_points) of the two chunks as a counting pass sizes them"""
    tops = [max(len(c) for c in clouds[:64]), len(clouds[64])]
    return [(n, max(1, min(t, native.ICP_MAX_POINTS) if capped else t)) for n, t in zip((64, 1), tops)]


def detected(n, mp, counted):
    head = [("simulate_batch_device", n)] + ([("detect_device", n, 0)] if counted else [])
    return head + [("detect_device", n, mp)]


def one_side_stream(streams):
    assert len(set(streams)) == 1 and isinstance(streams[0], int) and streams[0] != 0


def test_simulate_point_clouds_counts_then_fills_per_chunk(sim, poses, clouds, calls):
    noted, streams = calls
    out = sim.simulatePointClouds(poses, **CFAR)
    want = [c for n, mp in chunks(clouds, False) for c in detected(n, mp, True)] + [("synchronize",)]
    assert noted == want
    one_side_stream(streams)
    assert [c.tobytes() for c in out] == [c.tobytes() for c in clouds]
    del noted[:], streams[:]
    assert sim.simulatePointClouds(poses[:0], **CFAR) == [] and noted == [("synchronize",)] and streams[0] != 0     # no pose: the stream is still joined


@pytest.mark.parametrize("mode", ["cfar", "kstrongest", "cfar_compensated"])
def test_register_point_clouds_detects_then_registers_per_chunk(sim, poses, clouds, calls, mode):
    noted, streams = calls
    real, iterations = clouds[0], 3
    det = KSTRONGEST if mode == "kstrongest" else CFAR
    table = native.identity_sweep_table(1, 400)[0] if mode == "cfar_compensated" else None
    rec, fixed = sim.registerPointClouds(poses, real, detect=det, gate=1.0, iterations=iterations, compensate=table)
    sizes = [(64, 2 * 400), (1, 2 * 400)] if mode == "kstrongest" else chunks(clouds, True)
    want = []
    for n, mp in sizes:
        want += detected(n, mp, mode != "kstrongest")
        want += [("compensate_points_device", n, mp)] if table is not None else []
        want += [("register_points_device", n, mp, len(real), iterations)]
    assert noted == want + [("synchronize",)]
    one_side_stream(streams)
    assert rec.shape == (N_POSES,) and rec.dtype == native.ICP_DTYPE and fixed.shape == (N_POSES, 7)
    if mode != "kstrongest":                        # frame 0 is the real scan itself
        assert (rec["c"][0], rec["s"][0], rec["tx"][0], rec["ty"][0], rec["sse"][0]) == (1.0, 0.0, 0.0, 0.0, 0) and rec["n_matched"][0] == len(real)


@pytest.mark.parametrize("mode", ["cfar", "kstrongest"])
def test_build_likelihood_field_rasterizes_per_chunk_and_transforms_once(sim, poses, clouds, calls, mode):
    noted, streams = calls
    g = native.field_config(96, 80, 0.25, -12.0, -10.0)
    field = sim.buildLikelihoodField(poses, g, KSTRONGEST if mode == "kstrongest" else CFAR)
    sizes = [(64, 2 * 400), (1, 2 * 400)] if mode == "kstrongest" else chunks(clouds, True)
    want = []
    for n, mp in sizes:
        want += detected(n, mp, mode != "kstrongest") + [("rasterize_points_device", n, mp)]
    assert noted == want + [("distance_field_device", 1), ("synchronize",)]
    one_side_stream(streams)
    assert field.dtype == np.uint16 and field.shape == (80, 96) and field.min() == 0 and field.max() > 0
