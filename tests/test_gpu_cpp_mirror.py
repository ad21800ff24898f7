"""The C++ mirror's methods that no other program under tests/cpp/ runs (include/radarays_ros_amd/RadarHIP.hpp and marshal.hpp), driven by
tests/cpp/mirror_check.cpp in three runs ("sim", "notes", "img"), against
  * the ctypes path (native.Context) on the same inputs: the same library, the same beam, no noise -- bytes, no tolerance;
  * the numpy restatements, with the comparison (and so the bound) of each feature's own GPU test, imported from that test's file.
What the buffers of each C++ method must look like is read off include/radarays_mi355.h; the constants of the calls are the driver's."""
import os
import sys

import numpy as np
import pytest

import align_ref
import deskew_ref
import doppler_ref
import field_ref
import icp_ref
import labels_ref
import mirror_io as M
import notes_ref
import paths_ref
import place_ref
import shift_ref
from common import GOLDEN, golden_beams, mats_tuple
from radarays_ros_amd import native, params, radar, scenes

sys.path.insert(0, GOLDEN)
import gen_oracle_images as gen  # noqa: E402

from test_gpu_align import assert_records as assert_align_records      # noqa: E402  (TOL of tests/test_gpu_align.py)
from test_gpu_deskew import same_points                                # noqa: E402  (tests/test_gpu_deskew.py: bit for bit)
from test_gpu_icp import same_as_ref as same_icp_records               # noqa: E402  (tests/test_gpu_icp.py: bit for bit)
from test_gpu_paths import REL_DEV, rel_dev                            # noqa: E402  (tests/test_gpu_paths.py: four times the figure)
from test_gpu_place import assert_match                                # noqa: E402  (TOL of tests/test_gpu_place.py)
from test_gpu_shift import assert_records as assert_shift_records      # noqa: E402  (TOL of tests/test_gpu_shift.py)

pytestmark = pytest.mark.gpu

A = 400
N_CELLS, N_SAMPLES = 200, 50
ALL = native.METRIC_ALL
PROV_STRIDE, WAVE_STRIDE, DOP_STRIDE = 3, 60, 2          # each below the longest list of its kind (asserted where it is used)
DOP_GAIN, SENSOR_VEL = 0.0625, np.float32([6.0, -2.5, 0.25])
CHAIN_AZ = [0, 5, 123, 399]
NOTE_MASK = native.NOTE_DIRECT | native.NOTE_GHOST
SWEEP_GAIN, PIXEL, GATE = 0.03125, 0.25, 1.5             # exact in f32: the driver states the same literals
TIMEOUT = 120


def make_ctx(scene, mats, cfg, beams):
    c = native.Context(0)
    c.set_mesh(scene["verts"], scene["faces"], scene["face_object_id"])
    c.set_materials(mats, scene["object_materials"], 0)
    c.set_config(cfg)
    c.set_beam_samples(beams)
    return c


def run(exe, tmp, group, scene, mats, cfg, beams, pose, extra):
    inp, out = tmp / (group + "_in.bin"), tmp / (group + "_out.bin")
    M.write_sections(inp, M.scene_sections(group, scene, mats, cfg, beams, pose) + extra)
    r = M.run_driver(exe, [inp, out], timeout=TIMEOUT)
    assert r.returncode == 0, (r.stderr, r.stdout[-2000:])
    res = M.Results(M.read_sections(out))
    assert res.text("done") == group
    return res


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return M.build_driver(tmp_path_factory.mktemp("mirror"), native)


@pytest.fixture(scope="module")
def world():
    scene = gen.two_room_scene()                          # box12 with an inner penetrable box: two objects, three materials
    return scene, params.kaist_materials() + [params.PENETRABLE], scenes.default_pose("box12")


# ---- group "sim" ---------------------------------------------------------------------------------------------------------------------
def param_sets(mats):
    """4 sets: the loaded ones; other materials; fewer passes; another beam width (its beam drawn on the driver's seed 11)"""
    cur_bw = np.float32(10.0 * np.pi / 180.0)
    tables = [[m.astuple() for m in mats] for _ in range(4)]
    tables[1] = [(v, a * 0.5, d, s) for v, a, d, s in tables[1]]
    tables[3] = [(v, a, d + 0.125, s) for v, a, d, s in tables[3]]
    return np.float32(tables), np.int32([2, 2, 1, 2]), np.float32([cur_bw, cur_bw, cur_bw, np.float32(6.0 * np.pi / 180.0)])


@pytest.fixture(scope="module")
def sim(exe, world, tmp_path_factory):
    scene, mats, pose = world
    cfg = params.kaist_preset(n_cells=N_CELLS, n_samples=N_SAMPLES, n_reflections=2, ambient_noise=0, scroll_image=9)
    beams = golden_beams(N_SAMPLES)
    real = np.random.RandomState(3).randint(0, 256, (N_CELLS, A)).astype(np.uint8)
    tables, nref, bw = param_sets(mats)
    extra = [("prov_stride", np.uint64([PROV_STRIDE])), ("wave_stride", np.uint64([WAVE_STRIDE])), ("chain_az", np.int32(CHAIN_AZ)),
             ("dop", np.float32([DOP_GAIN, *SENSOR_VEL])), ("dop_stride", np.uint64([DOP_STRIDE])),
             ("ps.mats", tables), ("ps.nref", nref), ("ps.bw", bw), ("real", real)]
    res = run(exe, tmp_path_factory.mktemp("sim"), "sim", scene, mats, cfg, beams, pose, extra)
    ctx = make_ctx(scene, mats, cfg, beams)
    yield res, ctx, pose, cfg, real
    ctx.close()


def test_simulate_provenance(sim, oracle):
    res, ctx, pose, cfg, _ = sim
    plain = ctx.simulate(pose)[0]
    assert plain.any() and res.raw("sim0") == plain.tobytes()
    u8, lab, fac, ech, cnt = ctx.simulate_provenance(pose, echo_stride=0)
    assert ech is None and res.raw("pa.img") == u8.tobytes() == plain.tobytes()
    assert res.raw("pa.lab") == lab.tobytes() and res.raw("pa.fac") == fac.tobytes() and res.raw("pa.cnt") == cnt.tobytes()
    assert (lab != native.LABEL_NONE).any() and cnt.max() > PROV_STRIDE           # rows are truncated ...
    u8, lab, fac, ech, cnt2 = ctx.simulate_provenance(pose, echo_stride=PROV_STRIDE)
    assert np.array_equal(cnt2, cnt)                                              # ... and the counts stay true
    assert res.arr("pb.cnt", np.uint32).tobytes() == cnt.tobytes()
    got = res.arr("pb.ech", native.ECHO_SRC_DTYPE, (A, PROV_STRIDE))
    assert got.tobytes() == ech.tobytes() and res.raw("pb.img") == plain.tobytes()
    assert res.raw("pb.lab") == lab.tobytes() and res.raw("pb.fac") == fac.tobytes()
    # the truncated rows are the heads of the full ones
    full = ctx.simulate_provenance(pose)[3]
    for az in range(A):
        m = min(int(cnt[az]), PROV_STRIDE)
        assert got[az, :m].tobytes() == full[az, :m].tobytes(), az
    # the restatement (tests/labels_ref.py) on the full stream, exact as in
    # tests/test_gpu_labels.py::test_label_planes_are_the_restatement_of_the_exported_stream
    w, mode = labels_ref.weights(cfg, oracle)
    want_lab, want_fac = labels_ref.label_planes(full, cnt, cfg.n_cells, w, mode, cfg.scroll_image)
    for tag in ("pa", "pb"):
        got_lab, got_fac = res.arr(tag + ".lab", np.uint32, (N_CELLS, A)), res.arr(tag + ".fac", np.uint32, (N_CELLS, A))
        assert np.array_equal(got_lab, want_lab), (tag, np.argwhere(got_lab != want_lab)[:8])
        assert np.array_equal(got_fac, want_fac), (tag, np.argwhere(got_fac != want_fac)[:8])
    obj, pas, kind = native.unpack_info(want_lab[want_lab != native.LABEL_NONE])
    assert set(np.unique(obj)) == {0, 1} and (pas > 0).any()                      # both objects and ghosts show in the plane


def test_simulate_paths_and_path_to_echo(sim, world, oracle):
    res, ctx, pose, cfg, _ = sim
    u8, wav, cnt, pc = ctx.simulate_paths(pose)
    stride = int(res.arr("wa.stride", np.uint64, (1,))[0])
    assert stride == max(int(cnt.max()), 1) == wav.shape[1] and stride > WAVE_STRIDE
    assert res.raw("wa.img") == u8.tobytes() == res.raw("sim0")
    got = res.arr("wa.wav", native.WAVE_DTYPE, (A, stride))
    assert got.tobytes() == wav.tobytes() and res.raw("wa.cnt") == cnt.tobytes() and res.raw("wa.pas") == pc.tobytes()
    got_pc = res.arr("wa.pas", np.uint32, (A, native.WAVES_MAX_PASSES))
    assert np.array_equal(got_pc.sum(axis=1), res.arr("wa.cnt", np.uint32, (A,))) and (got_pc[:, 1] > 0).any() and not got_pc[:, 2:].any()
    u8, wav_m, cnt_m, pc_m = ctx.simulate_paths(pose, WAVE_STRIDE, map_frame=True)
    got_m = res.arr("wb.wav", native.WAVE_DTYPE, (A, WAVE_STRIDE))
    assert got_m.tobytes() == wav_m.tobytes() and res.raw("wb.cnt") == cnt_m.tobytes() == cnt.tobytes() and res.raw("wb.pas") == pc.tobytes()
    assert res.raw("wb.img") == u8.tobytes() and np.array_equal(got_m["o"][:, 0], np.broadcast_to(np.float32(pose[4:]), (A, 3)))
    assert not np.array_equal(got_m["d"][:, 0], got["d"][:, 0])                   # the map frame is another frame
    # pathToEcho on the returned rows against the Python twin's chain (radar.path_to_echo), every echo of the chosen azimuths
    n_echoes = ctx.simulate_provenance(pose, echo_stride=0)[4]
    chains = M.parse_chains(res.arr("chains", np.int32), with_az=True)
    assert sorted(chains) == [(az, k) for az in CHAIN_AZ for k in range(int(n_echoes[az]))] and len(chains) > 20
    longest = 0
    for (az, k), c in chains.items():
        assert c == radar.path_to_echo(wav[az, :cnt[az]], k)[0].tolist(), (az, k)
        longest = max(longest, len(c))
    assert longest == 2                                                           # ghosts of the second pass are among them
    # The restatement (tests/paths_ref.py: the bounce loop of one azimuth from the oracle's per-hit functions), with the comparison of
    # tests/test_gpu_paths.py::test_records_against_the_restatement.  Its bound is four times that file's REL_DEV; the figure of its case
    # "N" is used: the same three materials in nested boxes at three passes, where this scene has two, so a chain here meets no more
    # Fresnel splits (one ulp of acosf each, the source that file names) than a chain there.
    # Its echo log names the wave that owns each echo: walked back along the restatement's own `parent`, that is pathToEcho's chain.
    scene, mats, _ = world
    sc = oracle.Scene(scene["verts"], scene["faces"], scene["face_object_id"], use_bvh=0)
    worst = (0.0, -1, "", -1)
    for az in CHAIN_AZ:
        ref, rpc, echoes = paths_ref.trace_azimuth(oracle, sc, scene, mats_tuple(mats), scene["object_materials"], cfg, golden_beams(N_SAMPLES),
                                                   pose, az, A, False)
        assert len(ref) == cnt[az], (az, len(ref), cnt[az])
        mine = got[az, :cnt[az]]
        assert np.array_equal(got_pc[az, :len(rpc)], rpc), (az, got_pc[az], rpc)
        for f in ("parent", "material", "face", "info", "echo"):
            bad = np.flatnonzero(mine[f] != ref[f])
            assert bad.size == 0, (az, f, bad[:4], mine[f][bad[:4]], ref[f][bad[:4]])
        n0 = int(rpc[0])
        assert mine[:n0].tobytes() == ref[:n0].tobytes(), (az, "pass 0")
        dev, k, f = rel_dev(mine[n0:], ref[n0:])
        if dev > worst[0]:
            worst = (dev, n0 + k, f, az)
        assert len(echoes) == n_echoes[az], (az, len(echoes), n_echoes[az])
        for k in range(len(echoes)):
            chain, i = [], int(echoes["wave"][k])
            while i >= 0:
                chain.append(i)
                i = int(ref["parent"][i])
            assert chains[(az, k)] == chain[::-1], (az, k, chains[(az, k)], chain[::-1])
    print("C++ mirror paths rel dev: %.6e (wave %d, %s, azimuth %d); bound %.6e" % (worst + (4 * REL_DEV["N"],)))
    assert worst[0] <= 4 * REL_DEV["N"], worst


def test_simulate_doppler(sim, oracle):
    res, ctx, pose, cfg, _ = sim
    u8, _, vel, cel, cnt, vim = ctx.simulate_doppler(pose, None, DOP_GAIN)
    stride = int(res.arr("da.stride", np.uint64, (1,))[0])
    assert stride == max(int(cnt.max()), 1) == vel.shape[1] and stride > DOP_STRIDE
    assert res.raw("da.img") == u8.tobytes()
    assert res.arr("da.vel", np.float32, (A, stride)).tobytes() == vel.tobytes() and res.arr("da.cel", np.int32, (A, stride)).tobytes() == cel.tobytes()
    assert res.raw("da.cnt") == cnt.tobytes() and res.arr("da.vim", np.float32, (N_CELLS, A)).tobytes() == vim.tobytes()
    assert not vel.any()
    u8, _, vel, cel, cnt2, vim = ctx.simulate_doppler(pose, SENSOR_VEL, DOP_GAIN, DOP_STRIDE)
    assert np.array_equal(cnt2, cnt) and res.raw("db.cnt") == cnt.tobytes()
    assert res.arr("db.vel", np.float32, (A, DOP_STRIDE)).tobytes() == vel.tobytes()
    assert res.arr("db.cel", np.int32, (A, DOP_STRIDE)).tobytes() == cel.tobytes()
    assert res.raw("db.img") == u8.tobytes() != res.raw("sim0") and res.raw("db.vim") == vim.tobytes()
    assert np.abs(vel).max() > 1.0 and np.isfinite(vim).any()
    # The restatement (tests/doppler_ref.py) on the call's own wave and echo records, as tests/test_gpu_doppler.py::reference feeds it;
    # v_r by its f32 bits and cell' exactly (test_rates_and_cells_equal_the_definition), the velocity image against the winner column
    # with NaN exactly where nobody reaches the bin (test_image_and_velocity_image).  No twists: the C++ class cannot set any.
    wm, ws = ctx.simulate_paths(pose, map_frame=True)[1], ctx.simulate_paths(pose)[1]
    wcnt = ctx.simulate_paths(pose, 0)[2]
    ech = ctx.simulate_provenance(pose)[3]
    w, mode = labels_ref.weights(cfg, oracle)
    twists = np.zeros((ctx.n_objects, 6), np.float32)
    full_a = (res.arr("da.vel", np.float32, (A, stride)), res.arr("da.cel", np.int32, (A, stride)), res.arr("da.vim", np.float32, (N_CELLS, A)))
    cut_b = (res.arr("db.vel", np.float32, (A, DOP_STRIDE)), res.arr("db.cel", np.int32, (A, DOP_STRIDE)), res.arr("db.vim", np.float32, (N_CELLS, A)))
    moved = winners = 0
    for tag, v_s, (g_vel, g_cel, g_vim) in (("da", np.zeros(3, np.float32), full_a), ("db", SENSOR_VEL, cut_b)):
        for a in range(A):
            n = int(cnt[a])
            rv, rc, _ = doppler_ref.doppler(wm[a, :wcnt[a]], ws[a, :wcnt[a]], n, twists, v_s, DOP_GAIN, cfg.resolution)
            m = min(n, g_vel.shape[1])
            if tag == "da":                                                       # nothing moves: every rate is a zero
                assert not g_vel[a, :m].any() and not rv.any(), (tag, a)
            else:
                assert np.array_equal(g_vel[a, :m].view(np.uint32), rv[:m].view(np.uint32)), (tag, a)
            assert np.array_equal(g_cel[a, :m], rc[:m]), (tag, a)
            col = (cfg.scroll_image + a) % A
            want = doppler_ref.winner_column(rc, ech[a, :n]["strength"], rv, cfg.n_cells, w, mode)
            ok = ~np.isnan(want)
            assert np.array_equal(np.isnan(g_vim[:, col]), ~ok), (tag, a)
            assert np.array_equal(g_vim[:, col][ok], want[ok]) and (tag == "da" or np.array_equal(g_vim[:, col].view(np.uint32)[ok], want.view(np.uint32)[ok])), (tag, a)
            winners += int(ok.sum())
            moved += int((rc != ech[a, :n]["cell"]).sum()) if tag == "db" else 0
    assert moved > 0 and winners > 0


def test_simulate_param_sets_metrics(sim, world):
    res, ctx, pose, cfg, real = sim
    tables, nref, bw = param_sets(world[1])
    other = native.sample_cone_local(11, float(bw[3]), N_SAMPLES, cfg.beam_sample_dist, cfg.beam_sample_dist_normal_p_in_cone)
    sets = [{"materials": tables[k], "beam_dirs": other if k == 3 else None, "n_reflections": int(nref[k])} for k in range(4)]
    imgs, rec = ctx.simulate_param_sets(pose, sets, len(world[1]), ref_u8=real, want_images=True, metrics=ALL, win_size=7)
    got = res.arr("pm.rec", native.METRICS_DTYPE, (4,))
    assert got.tobytes() == rec.tobytes() and res.arr("pm.img", np.uint8, (4, N_CELLS, A)).tobytes() == imgs.tobytes()
    assert res.raw("pn.rec") == rec.tobytes()                                     # images null: the same records
    assert res.raw("pm.cmp") == ctx.compare_images(imgs, real, ALL, 7).tobytes() == rec.tobytes()
    assert imgs[0].tobytes() == res.raw("sim0") and len({imgs[k].tobytes() for k in range(4)}) == 4
    assert res.raw("sim1") == res.raw("sim0")                                     # the calls in between left the backend as it was


# ---- group "notes" -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def notes(exe, world, tmp_path_factory):
    scene, mats, pose = world
    cfg = params.kaist_preset(n_cells=64, n_samples=4, n_reflections=2, ambient_noise=0, resolution=0.3, scroll_image=9)
    beams = golden_beams(4)
    n = 65                                                # one more than RR_MAX_BATCH
    poses = np.stack([scenes.yaw_pose(1.0 - 0.03 * k, 1.5 + 0.02 * k, 0.2, 0.3 + 0.05 * k) for k in range(n)]).astype(np.float32)
    # what simulate() runs with (include_motion): one pose per azimuth, none of them a pose of the batch
    motion = np.stack([scenes.yaw_pose(-2.0 + 0.004 * a, 2.5 - 0.003 * a, 0.3, -0.4 + 0.001 * a) for a in range(A)]).astype(np.float32)
    res = run(exe, tmp_path_factory.mktemp("notes"), "notes", scene, mats, cfg, beams, pose, [("poses", poses), ("motion", motion)])
    ctx = make_ctx(scene, mats, cfg, beams)
    yield res, ctx, poses, cfg, motion
    ctx.close()


def test_simulate_annotations_across_a_chunk(notes):
    res, ctx, poses, cfg, motion = notes
    n, k = len(poses), ctx.n_objects
    assert k == 2
    n0, s0, i0 = ctx.simulate_batch_annotations(poses[:64], NOTE_MASK, want_images=True)        # the ctypes path in the ABI's chunks
    n1, s1, i1 = ctx.simulate_batch_annotations(poses[64:], NOTE_MASK, want_images=True)
    want_notes, want_skip, want_img = np.concatenate([n0, n1]), np.concatenate([s0, s1]), np.concatenate([i0, i1])
    for tag in ("an", "ai"):
        assert res.arr(tag + ".notes", native.NOTE_DTYPE, (n, k)).tobytes() == want_notes.tobytes(), tag
        assert res.arr(tag + ".skip", np.uint32, (n,)).tobytes() == want_skip.tobytes(), tag
    assert res.arr("ai.img", np.uint8, (n, 64, A)).tobytes() == want_img.tobytes()
    # frame 64 alone: the second chunk's outputs landed at their own offsets
    assert res.arr("a1.notes", native.NOTE_DTYPE, (1, k)).tobytes() == n1.tobytes() == res.arr("ai.notes", native.NOTE_DTYPE, (n, k))[64:].tobytes()
    assert res.raw("a1.skip") == s1.tobytes() and res.raw("a1.img") == i1.tobytes()
    assert want_notes["n_direct"].sum(axis=0).min() > 0 and len({want_img[f].tobytes() for f in (0, 63, 64)}) == 3
    # simulate() runs with the per-azimuth table before and after; the annotation frames in between are the poses' own: the call took
    # the table out (the ctypes frames above were made without one) and simulate() put it back
    plain = ctx.simulate(poses[64])[0]
    assert plain.tobytes() == i1.tobytes()
    ctx.set_motion_poses(motion)
    swept = ctx.simulate(poses[64])[0]
    ctx.set_motion_poses(None)
    assert res.raw("s0") == swept.tobytes() == res.raw("s1") and swept.tobytes() != plain.tobytes()
    assert res.text("rf.poses") == "poses must be [n][7]"
    # the restatement (tests/notes_ref.py) on the label plane of frame 64, with the comparison of tests/test_gpu_notes.py
    lab = ctx.simulate_provenance(poses[64], echo_stride=0)[1]
    g = ctx._rrcfg
    want, want_skipped, r_ext = notes_ref.annotate(lab[None], plain[None], k, NOTE_MASK, scroll=g.scroll_image, theta_min=g.theta_min,
                                                   theta_inc=g.theta_inc, resolution=g.resolution)
    notes_ref.assert_notes(res.arr("a1.notes", native.NOTE_DTYPE, (1, k)), want, r_ext)
    assert np.array_equal(res.arr("a1.skip", np.uint32, (1,)), want_skipped)


# ---- group "img" ---------------------------------------------------------------------------------------------------------------------
def offsets_of(cloud):
    """the offsets table rr_detect writes for a cloud sorted by column: points in the columns before c, the total last"""
    return np.searchsorted(cloud["column"], np.arange(A + 1), side="left").astype(np.uint32)


def field_cfg():
    return native.field_config(64, 48, 0.5, -16.0, -12.0, 20, 2)


@pytest.fixture(scope="module")
def img(exe, world, tmp_path_factory):
    scene, mats, pose = world
    cfg = params.kaist_preset(n_cells=N_CELLS, n_samples=4, n_reflections=1, ambient_noise=0, scroll_image=9)
    beams = golden_beams(4)
    rs = np.random.RandomState(4)
    imgs = rs.randint(0, 30, (6, N_CELLS, A)).astype(np.uint8)
    peaks = rs.rand(6, N_CELLS, A) < 0.02
    imgs[peaks] = rs.randint(80, 256, int(peaks.sum()))
    imgs[1] = np.roll(imgs[0], 7, axis=1)                 # an azimuth shift for the registration to find
    imgs[5] = np.roll(imgs[3], 30, axis=1)                # the sixth image: database entry 3 with its columns rolled (three sectors)
    az = np.stack([scenes.yaw_pose(0.002 * a, -0.001 * a, 0.0, 0.0002 * a) for a in range(A)]).astype(np.float32)
    ref = az[A // 2].copy()
    vel = np.float32([8.0, -3.0, 0.5])
    init = np.array([[2 * np.cos(0.02), 2 * np.sin(0.02), 0.1, -0.05], [1, 0, 0, 0], [np.cos(-0.01), np.sin(-0.01), 0.0, 0.1]], np.float64)
    fstates = np.array([[np.cos(0.1), np.sin(0.1), 0.5, -0.25], [np.cos(-0.2), np.sin(-0.2), -1.0, 0.75]], np.float64)
    yaw = rs.uniform(-0.1, 0.1, 33)
    hyps = np.stack([np.cos(yaw), np.sin(yaw), rs.uniform(-1, 1, 33), rs.uniform(-1, 1, 33)], axis=1).astype(np.float32)
    hyp_pose = scenes.yaw_pose(2.0, -1.0, 0.5, 0.7)
    extra = [("imgs", imgs), ("azposes", az), ("refpose", ref), ("svel", vel), ("icp_init", init), ("fstates", fstates), ("hyps", hyps),
             ("hyp_pose", hyp_pose)]
    res = run(exe, tmp_path_factory.mktemp("img"), "img", scene, mats, cfg, beams, pose, extra)
    ctx = make_ctx(scene, mats, cfg, beams)
    pts, offs = ctx.detect(imgs[0])
    inputs = dict(imgs=imgs, az=az, ref=ref, vel=vel, init=init, fstates=fstates, hyps=hyps, hyp_pose=hyp_pose, pts=pts[0], offs=offs)
    yield res, ctx, inputs
    ctx.close()


def test_align_images(img):
    res, ctx, x = img
    imgs, real = x["imgs"], x["imgs"][5]
    rec = ctx.align_images(imgs[:3], real)
    got = res.arr("al.rec", native.ALIGN_DTYPE, (3,))
    assert got.tobytes() == rec.tobytes() == res.raw("al.again")
    assert_align_records(got, None, [align_ref.align(im, real) for im in imgs[:3]])
    rec, curve = ctx.align_images(imgs[:3], real, 5, 64, want_curve=True)
    got, got_curve = res.arr("al2.rec", native.ALIGN_DTYPE, (3,)), res.arr("al2.cur", np.int64, (3, A))
    assert got.tobytes() == rec.tobytes() and got_curve.tobytes() == curve.tobytes()
    assert_align_records(got, got_curve, [align_ref.align(im, real, 5, 64) for im in imgs[:3]])
    assert "alignImages: every image must be n_cells x n_angles mono8" in res.text("rf.align")


def test_register_translation(img):
    res, ctx, x = img
    imgs, real = x["imgs"], x["imgs"][5]
    for tag, width, S, bilinear in (("sh", 65, 3, True), ("sh2", 64, 16, False)):
        cart = ctx.polar_to_cartesian(np.concatenate([imgs[:2], real[None]]), width, PIXEL, bilinear)      # n + 1 images, one conversion
        rec = ctx.shift_images(cart[:2], cart[2], S)
        got = res.arr(tag + ".rec", native.SHIFT_DTYPE, (2,))
        assert got.tobytes() == rec.tobytes(), tag
        box = shift_ref.box_sums(cart[2], S)
        assert_shift_records(got, None, None, [shift_ref.shift(im, cart[2], S, box=box) for im in cart[:2]])
    got = res.arr("sh.rec", native.SHIFT_DTYPE, (2,))
    assert res.raw("sh.again") == got.tobytes()
    want = np.stack([(got["dy"] + got["sub_dy"].astype(np.float64)) * float(np.float32(PIXEL)),
                     (got["dx"] + got["sub_dx"].astype(np.float64)) * float(np.float32(PIXEL))], axis=1)
    assert res.arr("sh.cor", np.float64, (2, 2)).tobytes() == want.tobytes()
    assert "registerTranslation: every image must be n_cells x n_angles mono8" in res.text("rf.shift")


def test_describe_images_and_localize(img):
    res, ctx, x = img
    imgs = x["imgs"]
    pc = (10, 40)
    db = ctx.describe_images(imgs[:5], pc)
    got_db = res.arr("pl.desc", np.uint8, (5, 10, 40))
    assert got_db.tobytes() == db.tobytes()
    assert np.array_equal(got_db, np.stack([place_ref.describe(im, 0, N_CELLS, 10, 40) for im in imgs[:5]]))
    q = ctx.describe_images(imgs[5], pc)
    for tag, k in (("pl.top3", 3), ("pl.top5", 5)):
        got = res.arr(tag, native.PLACE_DTYPE, (1, k))
        assert got.tobytes() == ctx.match_descriptors(q, db, k).tobytes(), tag
        assert_match(got, None, None, place_ref.match(q, db, k))
    top = res.arr("pl.top3", native.PLACE_DTYPE, (1, 3))[0, 0]
    assert top["index"] == 3 and top["sse"] == 0 and top["shift"] != 0            # entry 3, turned by three sectors
    assert res.raw("pl.again") == res.raw("pl.top3")
    assert "top_k must be 1..min(32, n_db)" in res.text("rf.topk")                # top_k > n_db: the ABI's own refusal
    assert "describeImages: every image must be n_cells x n_angles mono8" in res.text("rf.desc")
    assert "localize: the image must be n_cells x n_angles mono8 and the database n_db descriptors" in res.text("rf.db")


def test_sweep_compensation(img):
    res, ctx, x = img
    pts, offs, im0 = x["pts"], x["offs"], x["imgs"][0]
    assert len(pts) >= 200 and res.arr("dt.pts", native.POINT_DTYPE).tobytes() == pts.tobytes()
    g = ctx._rrcfg
    t0, t1 = ctx.sweep_table(x["az"], x["ref"]), ctx.sweep_table(x["az"], x["ref"], x["vel"], SWEEP_GAIN)
    got0, got1 = res.arr("sw.t0", native.SWEEP_DTYPE, (A,)), res.arr("sw.t1", native.SWEEP_DTYPE, (A,))
    assert got0.tobytes() == t0.tobytes() and got1.tobytes() == t1.tobytes()
    # the restatement, with the comparison of tests/test_gpu_deskew.py::test_table_matches_the_restatement
    want = deskew_ref.sweep_table(x["az"][None], x["ref"][None], x["vel"][None], SWEEP_GAIN, g.theta_min, g.theta_inc)[0]
    assert got1["q"].tobytes() == want["q"].tobytes() and got1["t"].tobytes() == want["t"].tobytes()
    assert np.all(got0["dr"].view(np.uint32) == 0)
    bound = (1e-6 * 1.0 + 1e-6) * abs(SWEEP_GAIN) * np.linalg.norm(x["vel"].astype(np.float64))
    assert np.all(np.abs(got1["dr"].astype(np.float64) - want["dr"]) <= bound) and np.abs(want["dr"]).max() > 0.1
    for tag, t in (("cp.0", t0), ("cp.1", t1)):
        got = res.arr(tag, native.POINT_DTYPE, (len(pts),))
        assert got.tobytes() == ctx.compensate_points([pts], offs, t)[0].tobytes(), tag
        same_points(got, deskew_ref.compensate_points(pts, t[0], g.scroll_image, g.resolution))
    assert res.raw("cp.again") == res.raw("cp.1") != res.raw("cp.0")
    for tag, bilinear, it in (("cc.1", False, 1), ("cc.2", True, 2)):
        got = res.arr(tag, np.uint8, (65, 65))
        assert got.tobytes() == ctx.polar_to_cartesian_sweep(im0, t1, 65, PIXEL, bilinear, it)[0].tobytes(), tag
        d = np.abs(got.astype(int) - deskew_ref.cartesian_sweep(im0, t1[0], 65, PIXEL, bilinear, it, scroll=g.scroll_image, theta_min=g.theta_min,
                                                                theta_inc=g.theta_inc, resolution=g.resolution))
        assert d.max() <= 1 and np.mean(d > 0) <= 1e-3, (tag, d.max(), np.mean(d > 0))      # tests/test_gpu_deskew.py's bound
    assert res.raw("cc.again") == res.raw("cc.2")
    assert res.text("rf.table") == "compensatePointClouds: the table must be [n_angles]"
    assert res.text("rf.sweep") == "sweepTable: the poses must be [n_angles][7]"
    for tag in ("rf.cart", "rf.carttab"):
        assert res.text(tag) == "compensatedCartesian: the image is not n_cells x n_angles mono8 or the table not [n_angles]"


def icp_clouds(ctx, x):
    cp1 = ctx.compensate_points([x["pts"]], x["offs"], ctx.sweep_table(x["az"], x["ref"], x["vel"], SWEEP_GAIN))[0]
    return [cp1[:65], cp1[:0], cp1[20:60]], x["pts"][:200]


def test_register_point_clouds(img):
    res, ctx, x = img
    clouds, tgt = icp_clouds(ctx, x)
    offs = np.stack([offsets_of(c) for c in clouds])      # a true offsets table per cloud: the C++ side's holds the totals only
    assert offs[:, -1].tolist() == [65, 0, 40]
    for tag, it, init in (("ic.a", 4, None), ("ic.b", 0, x["init"]), ("ic.c", 4, x["init"])):
        got = res.arr(tag, native.ICP_DTYPE, (3,))
        assert got.tobytes() == ctx.register_points(clouds, offs, tgt, init, GATE, it).tobytes(), tag
        same_icp_records(got, None, icp_ref.register(clouds, tgt, init, GATE, it)[0], None)
    a = res.arr("ic.a", native.ICP_DTYPE, (3,))
    assert a["n_matched"][0] >= 2 and a["n_matched"][1] == 0 and a["flags"][1] & 1        # the empty cloud: RR_ICP_DEGENERATE, no match
    assert res.raw("ic.again") == res.raw("ic.c") != res.raw("ic.a")
    # correctedPose against the Python function, to the bound tests/test_icp_host.py holds the same pair to (atol = 4e-6)
    rec = res.arr("ic.c", native.ICP_DTYPE, (3,))
    want = radar.RadarHIP._corrected_by(x["hyp_pose"][None].astype(np.float32), rec[:1])[0].astype(np.float32)
    got = res.arr("ic.pose", np.float32, (7,))
    assert np.allclose(got, want, rtol=0, atol=4e-6), np.abs(got - want).max()
    assert not np.array_equal(got, x["hyp_pose"])
    assert res.text("rf.init") == "registerPointClouds: a cloud of more than 65536 points, or init is not [n][4]"


def test_likelihood_field_and_scores(img):
    res, ctx, x = img
    pts, fc = x["pts"], field_cfg()
    keys = [pts[:65], pts[65:95]]
    offs = np.stack([offsets_of(c) for c in keys])
    fields = {}
    for tag, states in (("fd.a", x["fstates"]), ("fd.b", None)):
        occ = ctx.rasterize_points(keys, offs, fc, states)
        fields[tag] = ctx.distance_field(occ, fc)
        got = res.arr(tag, np.uint16, (48, 64))
        assert got.tobytes() == fields[tag].tobytes(), tag
        want_occ = field_ref.rasterize(keys, fc, states)
        assert np.array_equal(occ, want_occ) and want_occ.sum() > 40
        assert np.array_equal(got, field_ref.distance_field(want_occ, fc)), tag                 # tests/test_gpu_field.py: exact
    assert res.raw("fd.a") != res.raw("fd.b") and res.raw("fd.again") == res.raw("fd.a")
    scan = pts[100:165]
    assert len(scan) == 65 and len(x["hyps"]) == 33
    for tag, s in (("sc.a", scan), ("sc.e", scan[:0])):
        got = res.arr(tag, native.FIELD_DTYPE, (33,))
        assert got.tobytes() == ctx.score_poses(s, x["hyps"], fields["fd.a"], fc).tobytes(), tag
        assert got.tobytes() == field_ref.score(s, x["hyps"], fields["fd.a"], fc).tobytes(), tag
    assert res.arr("sc.a", native.FIELD_DTYPE, (33,))["n_in"].min() > 30 and not np.frombuffer(res.raw("sc.e"), np.uint8).any()
    assert res.raw("sc.again") == res.raw("sc.a")
    assert res.text("rf.states") == "buildLikelihoodField: no cloud, or states is not [n][4]"
    assert res.text("rf.hyps") == "scorePoses: states must be [n][4] and the field [height][width]"
