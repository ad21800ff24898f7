"""Cases and recorded results of the reference's OWN compiled loop (oracle/_ref/libradarays_refloop.so: RadarCPU.cpp and
radar_algorithms.cpp built against the behaving stand-ins of oracle/refshim/, `make -C oracle ref`).

Regenerate with:  python tests/golden/gen_refloop.py      (needs the reference checkout; about a minute)

The frame cases are the ones the GPU gate uses, built from the same generators (gen_oracle_images.py, the parameter list of
test_gpu_parity.test_config_variants, the presets of test_gpu_round5.py, fixtures.random_room_case).  Two things differ, and
only because the reference leaves no other way: the loop always renders the WHOLE sweep (the cases' azimuth windows are
dropped), and a Perlin noise offset is what the loop's random device makes of a seed, so the cases' own offsets are replaced
by offsets drawn that way (oracle.ref_noise_seeds: only seeds whose f64 offset is exactly an f32, since the build injects
f32 offsets).

What is stored (refloop_<case>.npz, each well under 160 KB): NOT the whole image but a FIXED SET OF 32 IMAGE COLUMNS
(`cols`, evenly spaced over the sweep; all of them where the sweep has fewer) of the reference loop's mono8 image, with the
beam table, the noise seeds and offsets and the pose(s).  The scene, materials and config are rebuilt from the generators.
refloop_fresnel_<k>.npz hold the C++ fresnel() outputs of the 11,000 cases of pyref_cases.py in chunks of 3,000,
refloop_functions.npz the C++ back_reflection_shader on the 3,624 cases of pyref_brdf.npy, the three denoiser tables,
Perlin values and DirectedWave::move results."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import gen_oracle_images as gen  # noqa: E402
import pyref_cases  # noqa: E402
from common import golden_beams, mats_tuple  # noqa: E402
from radarays_ros_amd import beams as beams_mod, params, scenes  # noqa: E402
from radarays_ros_amd.fixtures import random_room_case  # noqa: E402

N_COLS = 32
FRESNEL_CHUNK = 3000

# test_gpu_parity.test_config_variants' parameter list (tests/test_oracle_refloop.py checks that it still is)
VARIANTS = [
    dict(signal_denoising=0),
    dict(signal_denoising=3),
    dict(signal_denoising=2, signal_denoising_gaussian_width=200, signal_denoising_gaussian_mode=0.5),
    dict(record_multi_path=True, multipath_threshold=0.2),
    dict(record_multi_reflection=False),
    dict(ambient_noise=1),
    dict(n_cells=1000, resolution=0.2),
    dict(n_reflections=6),
]
FUZZ_SEEDS = list(range(12)) + [297, 454]          # test_gpu_parity._fuzz_seeds() without its environment extension


def _case(s, cfg, mats, beams, pose, objmat=None, n_angles=400, use_bvh=0):
    return dict(scene=s, cfg=cfg, mats=mats, objmat=s.get("object_materials") if objmat is None else objmat,
                beams=np.ascontiguousarray(beams, np.float32), pose=np.asarray(pose, np.float32), n_angles=n_angles,
                use_bvh=use_bvh)


def _preset_beams(cfg, seed=42):
    """the beams of test_gpu_round5._beam_of, from the package's host-side sampler"""
    import math
    return beams_mod.sample_cone_local_rad(cfg.beam_width * math.pi / 180.0, cfg.n_samples, cfg.beam_sample_dist,
                                           cfg.beam_sample_dist_normal_p_in_cone, seed)


def frame_cases():
    """name -> case, every frame case of tests/test_oracle_refloop.py"""
    two, kmats = gen.two_room_scene, lambda: params.kaist_materials() + [params.PENETRABLE]
    box_pose = scenes.default_pose("box12")
    C = {}
    s, cfg, mats, b, pose, _, _ = gen.case_config1()
    C["config1"] = _case(s, cfg, mats, b, pose)
    s, cfg, mats, b, pose, _, _ = gen.case_multibounce()
    C["multibounce"] = _case(s, cfg, mats, b, pose)
    s, cfg, mats, b, pose, _, _ = gen.case_noise()
    C["noise_scroll"] = _case(s, cfg, mats, b, pose)
    for k, kw in enumerate(VARIANTS):
        base = dict(n_reflections=3, ambient_noise=0)
        base.update(kw)
        C["variant%d_%s" % (k, sorted(kw)[0])] = _case(two(), params.kaist_preset(**base), kmats(), golden_beams(48), box_pose)
    # the three reference presets of test_gpu_round5.py, on scenes of a few thousand triangles
    cfg = params.laserlike_preset()
    C["preset_laserlike"] = _case(two(), cfg, kmats(), _preset_beams(cfg), box_pose)
    cfg = params.minimal_preset()
    s = scenes.heightfield_room(64, n_buildings=40, seed=3)
    z = scenes.default_pose(s["name"])[6]
    sweep = np.stack([scenes.yaw_pose(1.0 + 1.5 * t, 1.5 + 0.5 * t, z, 0.3 + 0.2 * t) for t in np.linspace(0, 1, 400)])
    C["preset_minimal_motion_noise"] = _case(s, cfg, kmats(), _preset_beams(cfg), sweep, use_bvh=1)
    cfg = params.kaist_preset()
    s = scenes.heightfield_room(40, n_buildings=30)
    C["preset_kaist_50_samples"] = _case(s, cfg, kmats(), _preset_beams(cfg), scenes.default_pose(s["name"]), use_bvh=1)
    s = scenes.oru4_like_scene()
    C["oru4_test_materials"] = _case(s, params.kaist_preset(ambient_noise=0, n_samples=40), params.oru4_test_materials(),
                                     golden_beams(40), scenes.default_pose(s["name"]), objmat=params.ORU4_OBJECT_MATERIALS)
    a = np.linspace(0.0, 1.0, 400)
    poses = np.stack([scenes.yaw_pose(1.0 + 2.0 * t, 1.5 - 1.0 * t, 0.2 + 0.5 * t, 0.3 + 0.4 * t) for t in a])
    C["include_motion"] = _case(two(), params.kaist_preset(n_reflections=3, ambient_noise=0, include_motion=True), kmats(),
                                golden_beams(32), poses)
    C["no_reflections"] = _case(two(), params.kaist_preset(n_reflections=0, ambient_noise=0), kmats(), golden_beams(8), box_pose)
    empty = {"verts": np.zeros((0, 3), np.float32), "faces": np.zeros((0, 3), np.uint32),
             "face_object_id": np.zeros(0, np.uint32), "object_materials": [1], "name": "empty"}
    C["empty_mesh"] = _case(empty, params.kaist_preset(n_reflections=2, ambient_noise=0), kmats(), golden_beams(8), box_pose)
    C["empty_mesh_noise"] = _case(empty, params.kaist_preset(n_reflections=1, ambient_noise=2), kmats(), golden_beams(8), box_pose)
    for n_angles, scroll in ((90, 8), (101, 7), (1, 0)):
        C["n_angles_%d" % n_angles] = _case(two(), params.kaist_preset(n_reflections=3, ambient_noise=2, scroll_image=scroll),
                                            kmats(), golden_beams(32), box_pose, n_angles=n_angles)
    for seed in FUZZ_SEEDS:
        s, cfg, mats, b, pose, _, _ = random_room_case(seed)
        C["fuzz_%d" % seed] = _case(s, cfg, mats, b, pose)
    for name, c in C.items():
        if not getattr(c["cfg"], "include_motion", False):
            assert c["pose"].shape == (7,), name
        elif c["pose"].shape == (7,):               # the .cfg default is include_motion = true: a table of one pose repeated
            c["pose"] = np.tile(c["pose"], (c["n_angles"], 1))
    return C


# the recorded subset (the issue's minimum and a little more); none of them draws the uniform stream of ambient_noise == 1,
# which the GPU defines for itself
RECORDED = ["config1", "multibounce", "noise_scroll", "variant0_signal_denoising", "variant1_signal_denoising",
            "variant2_signal_denoising", "variant3_multipath_threshold", "preset_minimal_motion_noise", "oru4_test_materials",
            "include_motion", "n_angles_101", "fuzz_1", "fuzz_5", "fuzz_6", "fuzz_9", "fuzz_454"]


def noise_inputs(O, name, case):
    """-> (seeds for the loop's random device | None, f32 offsets for the oracle and the GPU | None)"""
    if not case["cfg"].ambient_noise:
        return None, None
    start = 1000 + 7919 * (sum(ord(ch) for ch in name) % 1000)
    return O.ref_noise_seeds(start, case["n_angles"])


def run_reference(O, name, case):
    """the reference loop on a case -> (u8 image, seeds, offsets)"""
    c = case
    sc = O.Scene(c["scene"]["verts"], c["scene"]["faces"], c["scene"]["face_object_id"], use_bvh=c["use_bvh"])
    seeds, offs = noise_inputs(O, name, c)
    u8, log = O.ref_simulate(sc, mats_tuple(c["mats"]), c["objmat"], c["cfg"], c["beams"], c["pose"], noise_seeds=seeds,
                             n_angles=c["n_angles"])
    assert (len(log) == 0) if seeds is None else np.array_equal(log, seeds), name
    return u8, seeds, offs


def run_oracle(O, name, case, seeds, offs):
    c = case
    sc = O.Scene(c["scene"]["verts"], c["scene"]["faces"], c["scene"]["face_object_id"], use_bvh=c["use_bvh"])
    stream = O.ref_uniform_stream(seeds, c["cfg"].n_cells) if c["cfg"].ambient_noise == 1 else None
    u8, _, st = O.simulate(sc, mats_tuple(c["mats"]), c["objmat"], c["cfg"], c["beams"], c["pose"], noise_rnd=offs,
                           n_angles=c["n_angles"], want_f32=False, uniform_stream=stream)
    return u8, st


def stored_columns(n_angles):
    return np.unique(np.linspace(0, n_angles - 1, min(N_COLS, n_angles)).astype(np.int64))


def fresnel_inputs():
    """the 11,000 cases of pyref_cases.py, concatenated in family order: normals, directions, v1, v2"""
    th, v1, v2 = (np.concatenate(x) for x in zip(*[pyref_cases.cases(f) for f in pyref_cases.FAMILIES]))
    return np.tile(np.float32([[-1.0, 0.0, 0.0]]), (len(th), 1)), pyref_cases.direction(th), v1, v2


def denoiser_inputs(recorded=False):
    """every width 1..64 with every mode position 0..width-1, for the three kernels; the recorded subset keeps two mode
    positions per width (the presets' 0.35 and the last one) so that the file stays small"""
    if recorded:
        return [(kind, w, m) for kind in (1, 2, 3) for w in range(1, 65) for m in sorted({int(0.35 * w), w - 1})]
    return [(kind, w, m) for kind in (1, 2, 3) for w in range(1, 65) for m in range(w)]


def perlin_inputs():
    rs = np.random.RandomState(77)
    g = np.stack(np.meshgrid(np.linspace(-3.0, 20.0, 47), np.linspace(-2.5, 19.5, 45)), -1).reshape(-1, 2)
    far = rs.uniform(-1e6, 1e6, (500, 2))
    edge = np.float64([[0.0, 0.0], [255.0, 255.0], [256.0, 256.0], [-1.0, -1.0], [-0.0, 255.999999], [1e9, -1e9], [1000.0, 19.95]])
    xy = np.concatenate([g, far, edge])
    return np.concatenate([xy, np.zeros((len(xy), 1))], 1), rs.uniform(-300, 300, (300, 3))


def move_inputs():
    rs = np.random.RandomState(78)
    n = 500
    d = rs.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (rs.uniform(-50, 50, (n, 3)).astype(np.float32), d.astype(np.float32), rs.uniform(0, 400, n),
            rs.choice([0.3, 0.12, 0.03, 0.001], n), np.concatenate([rs.uniform(0, 300, n - 2), [0.001, 0.0]]))


def reference_functions(O):
    """the reference's C++ functions on the inputs above -> dict of arrays"""
    import ctypes as C
    R = O.refloop_lib()
    fp = C.POINTER(C.c_float)
    N, D, v1, v2 = fresnel_inputs()
    rd, td = np.zeros_like(D), np.zeros_like(D)
    re, te = np.zeros(len(D)), np.zeros(len(D))
    e1, e2 = C.c_double(), C.c_double()
    for i in range(len(D)):
        R.ref_fresnel(N[i].ctypes.data_as(fp), D[i].ctypes.data_as(fp), 1.0, 0.5, float(v1[i]), float(v2[i]),
                      rd[i].ctypes.data_as(fp), C.byref(e1), td[i].ctypes.data_as(fp), C.byref(e2))
        re[i], te[i] = e1.value, e2.value
    out = {"fresnel_rd": rd, "fresnel_re": re, "fresnel_td": td, "fresnel_te": te}
    X = np.load(os.path.join(HERE, "pyref_brdf.npy"))
    a, cx, w = X[:, 0], X[:, 1], X[:, 2]
    d = (np.float32(1.0) - a.astype(np.float32)).astype(np.float32)
    out["brdf"] = np.float32([R.ref_back_reflection_shader(np.float32(w[i]), 1.0, float(a[i]), float(d[i]), float(cx[i]))
                              for i in range(len(X))])
    tabs = []
    for kind, width, mode in denoiser_inputs(recorded=True):
        t = np.zeros(width, np.float32)
        getattr(R, "ref_make_denoiser_" + {1: "triangular", 2: "gaussian", 3: "maxwell_boltzmann"}[kind])(width, mode, t.ctypes.data_as(fp))
        tabs.append(t)
    out["denoisers"] = np.concatenate(tabs)
    p2, p3 = perlin_inputs()
    out["perlin"] = np.float64([R.ref_perlin_noise(*[float(v) for v in p]) for p in np.concatenate([p2, p3])])
    o, dd, t0, vel, dist = move_inputs()
    mo, mt = o.copy(), t0.copy()
    for i in range(len(o)):
        t = C.c_double(t0[i])
        R.ref_wave_move(mo[i].ctypes.data_as(fp), dd[i].ctypes.data_as(fp), C.byref(t), float(vel[i]), float(dist[i]))
        mt[i] = t.value
    out["move_orig"], out["move_time"] = mo, mt
    return out


def load_functions():
    """the committed function-level results, as reference_functions() returns them"""
    out = dict(np.load(os.path.join(HERE, "refloop_functions.npz")))
    parts, k = [], 0
    while os.path.exists(os.path.join(HERE, "refloop_fresnel_%d.npz" % k)):
        parts.append(np.load(os.path.join(HERE, "refloop_fresnel_%d.npz" % k))); k += 1
    for key in ("fresnel_rd", "fresnel_re", "fresnel_td", "fresnel_te"):
        out[key] = np.concatenate([p[key] for p in parts])
    return out


if __name__ == "__main__":
    from oracle import oracle as O
    O.build()
    assert O.refloop_lib() is not None, "needs the reference checkout (make -C oracle ref)"
    cases = frame_cases()
    for name in RECORDED:
        c = cases[name]
        assert c["cfg"].ambient_noise != 1, name
        u8, seeds, offs = run_reference(O, name, c)
        cols = stored_columns(c["n_angles"])
        keep = dict(cols=cols, u8=np.ascontiguousarray(u8[:, cols]), beams=c["beams"], pose=c["pose"])
        if seeds is not None:
            keep.update(noise_seeds=seeds, noise_offsets=offs)
        path = os.path.join(HERE, "refloop_%s.npz" % name)
        np.savez_compressed(path, **keep)
        print(name, u8.shape, "lit %.3f" % (u8 > 0).mean(), os.path.getsize(path), "bytes")
    F = reference_functions(O)
    n = len(F["fresnel_re"])
    for k in range(0, n, FRESNEL_CHUNK):
        np.savez_compressed(os.path.join(HERE, "refloop_fresnel_%d.npz" % (k // FRESNEL_CHUNK)),
                            **{key: F[key][k:k + FRESNEL_CHUNK] for key in ("fresnel_rd", "fresnel_re", "fresnel_td", "fresnel_te")})
    np.savez_compressed(os.path.join(HERE, "refloop_functions.npz"),
                        **{key: v for key, v in F.items() if not key.startswith("fresnel_")})
    for fn in sorted(os.listdir(HERE)):
        if fn.startswith("refloop_f"):
            print(fn, os.path.getsize(os.path.join(HERE, fn)), "bytes")
