"""The oracle against the reference's OWN C++ loop, compiled (oracle/_ref/libradarays_refloop.so: RadarCPU.cpp and
radar_algorithms.cpp of the checkout built against the behaving stand-ins of oracle/refshim/; `make -C oracle ref`).

Every GPU parity test compares a kernel with oracle/radarays_oracle.c, a restatement of RadarCPU::simulate.  Here the
restatement meets what it restates.  Both sides are scalar x86 code built with the same flags against the same libm, and
the nearest hit behind the stand-in simulator is the oracle's own orc_intersect, so the agreement asked for is EXACT: the
mono8 image byte for byte, returned floats and doubles bit for bit.  No tolerance anywhere in this file.

What stays outside, as DESIGN.md §2 item 6 already names it (the reference's behaviour there is undefined or its own
device's): the VARIATES of ambient_noise == 1 (the loop draws them from its random device; the oracle is handed the very
draws through its test hook, so everything around the stream is still compared), a beam distribution outside 0..3
(uninitialised radius), and the beam samples, which are an input on both sides.  A Perlin offset is whatever the loop's
random device makes of a seed (f64 `f32 draw * 1000.0`); the build injects f32 offsets, so the seeds used are those whose
offset is exactly an f32 (oracle.ref_noise_seeds).  No frame case is excluded.

The live tests need the library, i.e. the reference checkout at build time; where it is absent they skip, the
fixture-based tests below never do."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from common import GOLDEN

sys.path.insert(0, GOLDEN)
import gen_refloop as G  # noqa: E402

fp = C.POINTER(C.c_float)
CASES = G.frame_cases()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


@pytest.fixture(scope="module")
def refloop(oracle):
    if oracle.refloop_lib() is None:
        pytest.skip("oracle/_ref/libradarays_refloop.so is not built (no reference checkout on this machine)")
    return oracle.refloop_lib()


def test_the_case_list_is_the_gpu_gates():
    """the frame cases are built from the GPU gate's own lists: its config variants and its fuzz seeds, entry for entry"""
    import test_gpu_parity as P
    marks = [m for m in P.test_config_variants.pytestmark if m.name == "parametrize"]
    assert list(marks[0].args[1]) == G.VARIANTS
    env = os.environ.pop("RR_FUZZ_SEEDS", None)
    try:
        assert P._fuzz_seeds() == G.FUZZ_SEEDS
    finally:
        if env is not None:
            os.environ["RR_FUZZ_SEEDS"] = env
    marks = [m for m in P.test_other_azimuth_counts.pytestmark if m.name == "parametrize"]
    assert [a for a, _ in marks[0].args[1]] == [90, 101, 1]
    assert set(G.RECORDED) <= set(CASES) and len(CASES) == 36
    # the recorded subset is also the GPU's: none of it draws the ambient_noise == 1 stream, which each side defines itself
    assert all(CASES[n]["cfg"].ambient_noise != 1 for n in G.RECORDED)
    assert sum(n.startswith("fuzz_") for n in G.RECORDED) >= 4


@pytest.mark.parametrize("name", list(CASES))
def test_whole_frame_oracle_equals_the_reference_loop(oracle, refloop, name):
    c = CASES[name]
    r8, seeds, offs = G.run_reference(oracle, name, c)
    o8, st = G.run_oracle(oracle, name, c, seeds, offs)
    assert r8.shape == o8.shape == (c["cfg"].n_cells, c["n_angles"])
    diff = np.argwhere(r8 != o8)
    assert len(diff) == 0, (name, len(diff), diff[:5].tolist(), r8[tuple(diff[0])], o8[tuple(diff[0])])
    # the case is not vacuous: what it is named for really happens
    if name in ("no_reflections", "empty_mesh", "empty_mesh_noise"):
        assert not r8.any() and st["signals"] == 0
    elif not name.startswith("fuzz_"):
        assert r8.any() and st["signals"] > 0


def test_the_cases_reach_the_glue_the_issue_names(oracle):
    """every switch of the glue is on in some case: the four smear settings, multi-path echoes behind a second pass,
    multi-reflection off, both noise kinds, per-azimuth poses, a transmitting material"""
    kinds = {CASES[n]["cfg"].signal_denoising for n in CASES}
    assert kinds == {0, 1, 2, 3}
    assert any(CASES[n]["cfg"].record_multi_path and CASES[n]["cfg"].n_reflections > 1 for n in CASES)
    assert any(not CASES[n]["cfg"].record_multi_reflection for n in CASES)
    assert any(CASES[n]["cfg"].ambient_noise == 1 for n in CASES) and any(CASES[n]["cfg"].ambient_noise == 2 for n in CASES)
    assert any(CASES[n]["pose"].ndim == 2 for n in CASES)
    assert any(max(m.velocity for m in CASES[n]["mats"][1:]) > 0 for n in CASES)


def test_fresnel_bit_for_bit(oracle, refloop):
    """the 11,000 dense Fresnel / Snell cases through the C++ fresnel() against orc_fresnel"""
    L = oracle.lib()
    N, D, v1, v2 = G.fresnel_inputs()
    assert len(D) == 11000
    rd, td, ord_, otd = (np.zeros_like(D) for _ in range(4))
    re, te, ore, ote = (np.zeros(len(D)) for _ in range(4))
    a, b = C.c_double(), C.c_double()
    for i in range(len(D)):
        args = (N[i].ctypes.data_as(fp), D[i].ctypes.data_as(fp), 1.0, 0.5, float(v1[i]), float(v2[i]))
        refloop.ref_fresnel(*args, rd[i].ctypes.data_as(fp), C.byref(a), td[i].ctypes.data_as(fp), C.byref(b))
        re[i], te[i] = a.value, b.value
        L.orc_fresnel(*args, ord_[i].ctypes.data_as(fp), C.byref(a), otd[i].ctypes.data_as(fp), C.byref(b))
        ore[i], ote[i] = a.value, b.value
    for x, y in ((rd, ord_), (td, otd), (re, ore), (te, ote)):
        assert np.array_equal(_bits(x), _bits(y))
    assert np.isnan(re).any() and (td == 0).all(axis=1).any() and (td != 0).any(axis=1).any()     # NaN, total reflection, refraction
    # polarisation and energy other than the loop's start values
    for i in range(0, len(D), 97):
        args = (N[i].ctypes.data_as(fp), D[i].ctypes.data_as(fp), 0.37, 0.81, float(v1[i]), float(v2[i]))
        refloop.ref_fresnel(*args, rd[i].ctypes.data_as(fp), C.byref(a), td[i].ctypes.data_as(fp), C.byref(b))
        x = (a.value, b.value)
        L.orc_fresnel(*args, ord_[i].ctypes.data_as(fp), C.byref(a), otd[i].ctypes.data_as(fp), C.byref(b))
        assert _bits(np.float64(x)).tolist() == _bits(np.float64([a.value, b.value])).tolist()


def test_angles_and_shader_bit_for_bit(oracle, refloop):
    """get_incidence_angle / angle_between (the float acos overload) and back_reflection_shader on the
    3,624 BRDF cases"""
    L = oracle.lib()
    N, D, _, _ = G.fresnel_inputs()
    rs = np.random.RandomState(5)
    extra = rs.normal(size=(2000, 3)).astype(np.float32)
    extra /= np.linalg.norm(extra, axis=1, keepdims=True).astype(np.float32)
    for n, d in list(zip(N[::5], D[::5])) + list(zip(extra[:1000], extra[1000:])):
        want = refloop.ref_incidence_angle(n.ctypes.data_as(fp), d.ctypes.data_as(fp))
        got = L.orc_incidence_angle(n.ctypes.data_as(fp), d.ctypes.data_as(fp))
        assert _bits(np.float64([want])) == _bits(np.float64([got]))
        # angle_between(a, b) = acos(a . b) = the incidence angle of -a on b
        ab = refloop.ref_angle_between((-n).ctypes.data_as(fp), d.ctypes.data_as(fp))
        assert _bits(np.float64([ab])) == _bits(np.float64([L.orc_incidence_angle(d.ctypes.data_as(fp), n.ctypes.data_as(fp))]))
    X = np.load(os.path.join(GOLDEN, "pyref_brdf.npy"))
    assert len(X) == 3624
    a, cx, w = X[:, 0], X[:, 1], X[:, 2]
    d = (np.float32(1.0) - a.astype(np.float32)).astype(np.float32)
    for e in (1.0, 0.37):
        want = np.float32([refloop.ref_back_reflection_shader(np.float32(w[i]), e, float(a[i]), float(d[i]), float(cx[i])) for i in range(len(X))])
        got = np.float32([L.orc_back_reflection_shader(np.float32(w[i]), e, float(a[i]), float(d[i]), float(cx[i])) for i in range(len(X))])
        assert np.array_equal(_bits(want), _bits(got))


def test_denoiser_tables_bit_for_bit(oracle, refloop):
    """widths 1..64, every mode position, the three kernels (mode 0 divides by zero in the triangular ramps: NaN / inf on
    both sides, bit for bit)"""
    for kind, width, mode in G.denoiser_inputs():
        want = np.zeros(width, np.float32)
        getattr(refloop, "ref_make_denoiser_" + {1: "triangular", 2: "gaussian", 3: "maxwell_boltzmann"}[kind])(width, mode, want.ctypes.data_as(fp))
        got = oracle.make_denoiser(kind, width, mode)
        assert np.array_equal(_bits(want), _bits(got)), (kind, width, mode, want, got)


def test_perlin_and_move_bit_for_bit(oracle, refloop):
    p2, p3 = G.perlin_inputs()
    for p in np.concatenate([p2, p3]):
        p = [float(v) for v in p]
        assert _bits(np.float64([refloop.ref_perlin_noise(*p)])) == _bits(np.float64([oracle.perlin_noise(*p)])), p
    L = oracle.lib()
    o, d, t0, vel, dist = G.move_inputs()
    for i in range(len(o)):
        a, b = o[i].copy(), o[i].copy()
        ta, tb = C.c_double(t0[i]), C.c_double(t0[i])
        refloop.ref_wave_move(a.ctypes.data_as(fp), d[i].ctypes.data_as(fp), C.byref(ta), float(vel[i]), float(dist[i]))
        L.orc_wave_move(b.ctypes.data_as(fp), d[i].ctypes.data_as(fp), C.byref(tb), float(vel[i]), float(dist[i]))
        assert np.array_equal(_bits(a), _bits(b)) and _bits(np.float64([ta.value])) == _bits(np.float64([tb.value]))


@pytest.mark.parametrize("sample_dist", [0, 1, 2, 3])
def test_sample_cone_local_bit_for_bit(oracle, refloop, sample_dist):
    """the reference's sample_cone_local with its random device handing out a known seed, against the oracle's twin fed the
    variates that seed produces"""
    import math
    for seed, width_deg, n, p in ((42, 10.0, 200, 0.8), (7, 2.0, 10, 0.95), (123456, 1e-4, 1, 0.8), (9, 45.0, 64, 0.5)):
        dirs, u, r = (np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32))
        w = np.float32(width_deg * math.pi / 180.0)
        rc = refloop.ref_sample_cone_local(seed, w, n, sample_dist, p, dirs.ctypes.data_as(fp), u.ctypes.data_as(fp), r.ctypes.data_as(fp))
        assert rc == 0
        got = oracle.sample_cone_local(w, sample_dist, p, u, r)
        assert np.array_equal(_bits(dirs), _bits(got)), (seed, sample_dist)


# ---- recorded results: no skip, no checkout needed ----------------------------------------------------------------------

@pytest.mark.parametrize("name", G.RECORDED)
def test_recorded_frames_match_the_oracle_and_a_fresh_reference_run(oracle, name):
    """tests/golden/refloop_<case>.npz (32 columns of the reference loop's image) against the oracle, and -- where the
    library is built -- against a fresh run of the reference loop, so that a stale fixture fails"""
    c = CASES[name]
    f = np.load(os.path.join(GOLDEN, "refloop_%s.npz" % name))
    assert np.array_equal(f["cols"], G.stored_columns(c["n_angles"])) and f["u8"].shape == (c["cfg"].n_cells, len(f["cols"]))
    assert np.array_equal(_bits(f["beams"]), _bits(c["beams"])) and np.array_equal(_bits(f["pose"]), _bits(c["pose"]))
    seeds = f["noise_seeds"] if "noise_seeds" in f else None
    offs = f["noise_offsets"] if "noise_offsets" in f else None
    assert (seeds is not None) == bool(c["cfg"].ambient_noise)
    o8, _ = G.run_oracle(oracle, name, c, seeds, offs)
    assert np.array_equal(o8[:, f["cols"]], f["u8"])
    assert f["u8"].any()
    if oracle.refloop_lib() is not None:
        r8, s2, o2 = G.run_reference(oracle, name, c)
        assert np.array_equal(r8[:, f["cols"]], f["u8"])
        if seeds is not None:
            assert np.array_equal(s2, seeds) and np.array_equal(_bits(o2), _bits(offs))


def test_recorded_functions_match_the_oracle_and_a_fresh_reference_run(oracle):
    F = G.load_functions()
    L = oracle.lib()
    N, D, v1, v2 = G.fresnel_inputs()
    assert F["fresnel_rd"].shape == (11000, 3) and F["brdf"].shape == (3624,)
    ord_, otd = np.zeros_like(D), np.zeros_like(D)
    ore, ote = np.zeros(len(D)), np.zeros(len(D))
    a, b = C.c_double(), C.c_double()
    for i in range(len(D)):
        L.orc_fresnel(N[i].ctypes.data_as(fp), D[i].ctypes.data_as(fp), 1.0, 0.5, float(v1[i]), float(v2[i]),
                      ord_[i].ctypes.data_as(fp), C.byref(a), otd[i].ctypes.data_as(fp), C.byref(b))
        ore[i], ote[i] = a.value, b.value
    for key, got in (("fresnel_rd", ord_), ("fresnel_td", otd), ("fresnel_re", ore), ("fresnel_te", ote)):
        assert np.array_equal(_bits(F[key]), _bits(got)), key
    X = np.load(os.path.join(GOLDEN, "pyref_brdf.npy"))
    d = (np.float32(1.0) - X[:, 0].astype(np.float32)).astype(np.float32)
    got = np.float32([L.orc_back_reflection_shader(np.float32(X[i, 2]), 1.0, float(X[i, 0]), float(d[i]), float(X[i, 1])) for i in range(len(X))])
    assert np.array_equal(_bits(F["brdf"]), _bits(got))
    tabs = np.concatenate([oracle.make_denoiser(k, w, m) for k, w, m in G.denoiser_inputs(recorded=True)])
    assert np.array_equal(_bits(F["denoisers"]), _bits(tabs))
    p2, p3 = G.perlin_inputs()
    got = np.float64([oracle.perlin_noise(*[float(v) for v in p]) for p in np.concatenate([p2, p3])])
    assert np.array_equal(_bits(F["perlin"]), _bits(got))
    if oracle.refloop_lib() is not None:
        fresh = G.reference_functions(oracle)
        assert set(fresh) == set(F)
        for key in fresh:
            assert np.array_equal(_bits(fresh[key]), _bits(F[key])), key
