"""The HIP path against the REFERENCE LOOP'S recorded bytes (tests/golden/refloop_*.npz: the mono8 columns, beam tables and
noise offsets tests/golden/gen_refloop.py recorded from the reference's own compiled RadarCPU::simulate, and its C++
fresnel() / back_reflection_shader outputs) -- not against the oracle.  The gate is the project's image gate, taken from
tests/test_gpu_parity.py: u8 off by at most 1, on at most U8_MISMATCH_TOL of the compared pixels.  Reads tests/golden/ only."""
import math
import os
import sys

import numpy as np
import pytest

from common import GOLDEN
from test_gpu_parity import U8_MISMATCH_TOL

sys.path.insert(0, GOLDEN)
import gen_refloop as G  # noqa: E402
import pyref_cases  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", G.RECORDED)
def test_frames_against_the_reference_loops_recorded_bytes(native_lib, name):
    c = G.frame_cases()[name]
    f = np.load(os.path.join(GOLDEN, "refloop_%s.npz" % name))
    s, cfg, n_angles = c["scene"], c["cfg"], c["n_angles"]
    ctx = native_lib.Context(0)
    ctx.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    ctx.set_materials(c["mats"], c["objmat"], 0)
    ctx.set_config(cfg, n_angles)
    ctx.set_beam_samples(f["beams"])
    if cfg.ambient_noise:
        ctx.set_noise_offsets(f["noise_offsets"])
    pose = f["pose"]
    if pose.ndim == 2:
        ctx.set_motion_poses(pose)
    g8, _, st = ctx.simulate(pose[0] if pose.ndim == 2 else pose, 0, n_angles)
    ctx.close()
    assert st["overflow"] == 0 and g8.shape == (cfg.n_cells, n_angles)
    d = np.abs(g8[:, f["cols"]].astype(np.int32) - f["u8"].astype(np.int32))
    print(name, "u8_max", int(d.max()), "mismatch", float((d > 0).mean()), "of", d.size)
    assert d.max() <= 1 and (d > 0).mean() <= U8_MISMATCH_TOL, (name, int(d.max()), float((d > 0).mean()))


def test_fresnel_split_against_the_recorded_cpp_outputs(native_lib):
    """rr_debug_fresnel on the 11,000 cases against the C++ fresnel()'s recorded outputs, by the laws
    test_gpu_round6.test_gpu_fresnel_split_against_the_oracle_on_the_reference_derived_cases applies against the oracle"""
    F = G.load_functions()
    c = native_lib.Context(0)
    k0, report = 0, {}
    for fam in pyref_cases.FAMILIES:
        th, v1, v2 = pyref_cases.cases(fam)
        sl = slice(k0, k0 + len(th)); k0 += len(th)
        D = pyref_cases.direction(th)
        Nn = np.tile(np.array([[-1.0, 0.0, 0.0]], np.float32), (len(th), 1))
        rd, re, td, te = c.debug_fresnel(Nn, D, 1.0, v1, v2.astype(np.float32))
        ord_, ore, otd32 = F["fresnel_rd"][sl], F["fresnel_re"][sl], F["fresnel_td"][sl]
        assert np.array_equal(rd.view(np.uint32), ord_.view(np.uint32)), fam
        tr = np.any(otd32 != 0, axis=1)
        flip = np.any(td != 0, axis=1) != tr
        for i in np.nonzero(flip)[0]:
            assert v2[i] > v1[i] and abs(th[i] - math.asin(v1[i] / v2[i])) < 1e-6, (fam, i)
        same = np.all(td.view(np.uint32) == otd32.view(np.uint32), axis=1) & ~flip
        for i in np.nonzero(~same & ~flip)[0]:
            n12 = v2[i] / v1[i]
            ct = max(math.cos(math.asin(min(1.0, math.sin(th[i]) * n12))), 1e-4)
            assert np.abs(td[i] - otd32[i]).max() < 2e-7 + 2e-7 * n12 * n12 / ct, (fam, i, td[i], otd32[i])
        nan_o, nan_g = np.isnan(ore), np.isnan(re)
        ok = same & ~nan_o & ~nan_g
        tight = np.abs(re[ok] - ore[ok]) < 1e-12
        report[fam] = (len(th), int(flip.sum()), float(same.mean()), float(tight.mean()), int((nan_o != nan_g).sum()),
                       float(np.abs(re[ok] - ore[ok]).max()))
        assert same.mean() > 0.93 and tight.mean() > 0.93, report
        assert (nan_o != nan_g).sum() <= 0.02 * len(th), report
        loose = ok & (np.minimum(th, np.where(tr, np.arcsin(np.minimum(1.0, np.sin(th) * v2 / np.maximum(v1, 1e-9))), np.pi / 2)) > 5e-3)
        assert not loose.any() or np.abs(re[loose] - ore[loose]).max() < 2e-5, report
    assert k0 == len(F["fresnel_re"]) == 11000
    print("fresnel GPU vs recorded C++ (cases, flips, dir bit-equal, energy < 1e-12, NaN mismatches, max |dE|):", report)
    c.close()


def test_brdf_against_the_recorded_cpp_outputs(native_lib):
    """rr_debug_brdf on the 3,624 cases against the C++ back_reflection_shader's recorded floats, by law (a) of
    test_gpu_round6.test_gpu_brdf_against_the_oracle_on_the_reference_derived_cases"""
    X = np.load(os.path.join(GOLDEN, "pyref_brdf.npy"))
    a, cx, w = X[:, 0], X[:, 1], X[:, 2]
    d = (np.float32(1.0) - a.astype(np.float32)).astype(np.float32)
    ref = G.load_functions()["brdf"].astype(np.float64)
    c = native_lib.Context(0)
    got = c.debug_brdf(w, 1.0, a, d, cx).astype(np.float64)
    c.close()
    lobe = (1.0 - a) * np.cos(w) ** cx
    dev = np.abs(got - ref)
    law_a = 1.5e-7 * np.maximum(ref, 1e-30) + lobe * (2.5e-7 + 1.3e-7 * cx)
    same = float((got.astype(np.float32) == ref.astype(np.float32)).mean())
    print("brdf GPU vs recorded C++: bit-equal %.4f, max |d| %.3g" % (same, dev.max()))
    assert same >= 0.90, same
    assert (dev <= law_a + 1e-12).all(), (dev.max(), X[np.argmax(dev - law_a)])
