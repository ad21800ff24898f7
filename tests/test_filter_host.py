"""The particle filter step without a GPU: the numpy restatement (tests/filter_ref.py) equals a brute-force version in Python integers and
has the properties of systematic resampling; the variates have their moments and the move keeps (c, s) a unit vector; the ABI version has
not moved (names, prototypes and the records' layout: tests/test_abi.py); configs are range-checked and the wrappers refuse bad
arguments before any call into the library; the facades have the call and the C++ method compiles; rr_filter.hip is in the library build
with each launcher declared once and its kernels use no scratch memory; and the closed loop holds on the oracle's images."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import field_ref as F
import filter_ref as R
from radarays_ros_amd import native, params, radar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radarays_ros_amd", "csrc")
NEW = ["rr_filter_resample_device", "rr_filter_resample", "rr_filter_move_device", "rr_filter_move", "rr_filter_tile_sizes"]


def cases():
    """(sum_d2, table, quantum, phase, n_out) small enough for the brute force"""
    rs = np.random.RandomState(5)
    out = []
    for n, n_table, quantum, phase, n_out in ((1, 1, 1, 0, 1), (2, 4, 3, 1 << 23, 5), (17, 8, 1, (1 << 24) - 1, 17), (33, 16, 7, 12345, 9),
                                              (64, 4096, 1 << 31, 999, 128), (40, 5, 2, 0, 40)):
        d2 = rs.randint(0, 1 << 33 if quantum > 1000 else 64, n).astype(np.uint64) + np.uint64(1 << 33 if n == 17 else 0)
        out.append((d2, native.filter_weight_table(2.0, min(quantum, 64), n_table), quantum, phase, n_out))
    return out


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_brute_force():
    for d2, table, quantum, phase, n_out in cases():
        cum, anc, s = R.resample(d2, table, quantum, phase, n_out)
        bcum, banc, bs = R.resample_brute(d2, table, quantum, phase, n_out)
        assert cum.dtype == np.uint64 and anc.dtype == np.uint32 and s.dtype == R.SUMMARY_DTYPE == native.FILTER_SUMMARY_DTYPE
        assert [int(x) for x in cum] == bcum and [int(x) for x in anc] == banc
        assert {k: int(s[k]) for k in s.dtype.names} == bs
    assert R.variates(7, 3, 50).tolist() == R.variates_brute(7, 3, 50)
    assert R.variates(0xffffffff, 0xfffffffe, 9).tolist() == R.variates_brute(0xffffffff, 0xfffffffe, 9)


def test_systematic_resampling_properties():
    rs = np.random.RandomState(9)
    d2 = rs.randint(0, 400, 3000).astype(np.uint64)
    table = native.filter_weight_table(4.0, 2, 128)                      # 128 * 2 < 400: the worst particles sit on the last entry
    table[-1] = 0                                                        # ... which weighs nothing
    for n_out, phase in ((3000, 0), (1500, 77777), (6000, (1 << 24) - 1)):
        cum, anc, s = R.resample(d2, table, 2, phase, n_out)
        w, _, _ = R.weights(d2, table, 2)
        assert np.all(np.diff(anc.astype(np.int64)) >= 0)                # non-decreasing
        copies = np.bincount(anc, minlength=len(d2))
        assert np.all(np.abs(copies - n_out * w.astype(np.float64) / float(s["total_weight"])) < 1.0)
        assert (w == 0).sum() > 100 and np.all(copies[w == 0] == 0)      # a zero-weight particle is never drawn
        assert int(s["n_unique"]) == len(np.unique(anc))
    # one dominant particle takes every draw
    d2 = np.full(500, 1000, np.uint64)
    d2[123] = 0
    t = np.zeros(16, np.uint16)
    t[0] = 9
    cum, anc, s = R.resample(d2, t, 1, 4242, 700)
    assert np.all(anc == 123) and int(s["n_unique"]) == 1 and int(s["best"]) == 123 and int(s["total_weight"]) == 9 and int(s["sum_w2"]) == 81
    # W == 0: n - 1 everywhere, by definition
    cum, anc, s = R.resample(d2, np.zeros(16, np.uint16), 1, 4242, 700)
    assert np.all(cum == 0) and np.all(anc == 499) and int(s["total_weight"]) == 0 and int(s["n_unique"]) == 1 and int(s["best"]) == 123


def test_variates_have_their_moments():
    v = R.variates(2024, 11, 1 << 20).astype(np.float64)
    assert v.min() >= -131070 and v.max() <= 131070
    for k in range(3):
        assert abs(v[:, k].mean()) <= 0.01 * math.sqrt(R.VARIATE_VAR)    # "within 1 % of 0": of the standard deviation, the only scale there is
        assert abs(v[:, k].var() / R.VARIATE_VAR - 1.0) <= 0.01
    assert abs(np.corrcoef(v.T)[0, 1]) < 0.01
    assert abs(native.FILTER_VARIATE_STD ** 2 / R.VARIATE_VAR - 1.0) < 1e-12


def test_the_move_keeps_a_unit_vector_and_copies_at_sigma_zero():
    rs = np.random.RandomState(3)
    yaw = rs.uniform(-math.pi, math.pi, 4096)
    st = np.stack([np.cos(yaw), np.sin(yaw), rs.uniform(-50, 50, 4096), rs.uniform(-50, 50, 4096)], axis=1).astype(np.float32)
    fc = native.filter_config(0.05, math.radians(0.5), 1, 1)
    inc = (math.cos(0.1), math.sin(0.1), 0.3, -0.2)
    out = R.move(st, None, inc, fc.sigma_xy, fc.sigma_t, 1, 2)
    norm2 = out[:, 0].astype(np.float64) ** 2 + out[:, 1].astype(np.float64) ** 2
    assert np.all(np.abs(norm2 - 1.0) <= 2 * np.finfo(np.float32).eps)   # within 2 ulp of 1
    # the diffusion has the deviations that were asked for
    still = R.move(st, None, (1, 0, 0, 0), fc.sigma_xy, fc.sigma_t, 1, 2)
    d = (still[:, 2:].astype(np.float64) - st[:, 2:]).ravel()
    assert abs(d.std() / 0.05 - 1.0) < 0.05
    dyaw = np.arctan2(still[:, 1].astype(np.float64), still[:, 0]) - np.arctan2(st[:, 1].astype(np.float64), st[:, 0])
    dyaw = np.arctan2(np.sin(dyaw), np.cos(dyaw))
    assert abs(dyaw.std() / math.radians(0.5) - 1.0) < 0.05
    # sigma 0 and no increment: the states, gathered and renormalised
    anc = rs.randint(0, 4096, 100).astype(np.uint32)
    same = R.move(st, anc, (1, 0, 0, 0), 0.0, 0.0, 5, 6)
    assert np.array_equal(same[:, 2:], st[anc][:, 2:]) and np.allclose(same[:, :2], st[anc][:, :2], atol=2e-7)
    nan = st.copy()
    nan[7] = np.nan
    assert np.all(np.isnan(R.move(nan, None, inc, fc.sigma_xy, fc.sigma_t, 1, 2)[7]))


# ---- the ABI and the wrappers ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_the_abi_version_has_not_moved(native_lib):
    native_lib.build()
    L = native_lib.lib()
    for n in NEW:
        assert hasattr(L, n) and n in native_lib.PROTOTYPES, n
    assert L.rr_abi_version() == 7
    scan_tile, draws, search_tile = native.filter_tile_sizes()
    assert scan_tile >= 64 and scan_tile * scan_tile >= 1 << 22 and draws in (64, 128, 256, 512, 1024) and 0 <= search_tile <= 8192
    assert native.FILTER_SUMMARY_DTYPE.itemsize == 32 and native.FILTER_CONFIG_DTYPE.itemsize == 32


def test_filter_config_is_range_checked():
    c = native.filter_config(0.05, math.radians(0.5), 1 << 31, 4096, (1 << 24) - 1, 0xffffffff, 7)
    assert (c.quantum, c.n_table, c.phase, c.seed, c.step, c.reserved) == (1 << 31, 4096, (1 << 24) - 1, 0xffffffff, 7, 0)
    assert abs(c.sigma_xy * native.FILTER_VARIATE_STD / 0.05 - 1) < 1e-6
    assert abs(c.sigma_t * native.FILTER_VARIATE_STD / math.tan(math.radians(0.25)) - 1) < 1e-6
    good = dict(sigma_xy_m=0.1, sigma_yaw_rad=0.01, quantum=4, n_table=16, phase=3, seed=1, step=2)
    for bad in (dict(sigma_xy_m=-0.1), dict(sigma_xy_m=float("nan")), dict(sigma_xy_m=float("inf")), dict(sigma_yaw_rad=-1.0), dict(sigma_yaw_rad=4.0),
                dict(sigma_yaw_rad="a"), dict(quantum=0), dict(quantum=(1 << 31) + 1), dict(quantum=1.5), dict(n_table=0), dict(n_table=4097),
                dict(phase=-1), dict(phase=1 << 24), dict(seed=-1), dict(seed=1 << 32), dict(step=1 << 32), dict(step=True)):
        with pytest.raises(ValueError):
            native.filter_config(**dict(good, **bad))
    with pytest.raises(ValueError):
        native._filter_cfg(native.RRFilterConfig(1, 1, 0, 0, 0, 0.0, 0.0, 1))             # reserved
    with pytest.raises(ValueError):
        native._filter_cfg(native.RRFilterConfig(1, 1, 0, 0, 0, float("nan"), 0.0, 0))
    with pytest.raises(ValueError):
        native._filter_cfg("config")
    t = native.filter_weight_table(1e-3, 1, 8)
    assert t.dtype == np.uint16 and t[0] == 65535 and np.all(t[1:] == 0)
    t = native.filter_weight_table(2.0, 4, 64)
    assert np.all(np.diff(t.astype(np.int64)) <= 0) and t[1] == round(65535 * math.exp(-4 / 8.0))
    for bad in ((0.0, 1, 8), (float("nan"), 1, 8), (1.0, 0, 8), (1.0, 1, 0), (1.0, 1, 4097)):
        with pytest.raises(ValueError):
            native.filter_weight_table(*bad)


def _unopened():
    o = native.Context.__new__(native.Context)
    o._h = None
    o._L = None
    o.cfg = params.RadarModelConfig(n_cells=64)
    o.n_angles = 16
    return o


def test_wrappers_refuse_bad_arguments_before_the_library():
    o = _unopened()
    fc = native.filter_config(0.1, 0.01, 1, 4)
    recs, table = np.zeros(5, native.FIELD_DTYPE), np.ones(4, np.uint16)
    for bad in ((np.zeros(5, np.uint64), table, 5, fc), (np.zeros((5, 1), native.FIELD_DTYPE), table, 5, fc), (recs[:0], table, 5, fc),
                (recs, table[:3], 5, fc), (recs, table.astype(np.int32), 5, fc), (recs, table, 0, fc), (recs, table, (1 << 22) + 1, fc),
                (recs, table, 5, "cfg"), (recs, table, 5, dict(quantum=0))):
        with pytest.raises(ValueError):
            o.filter_resample(*bad)
    st = np.zeros((5, 4), np.float32)
    for bad in ((np.zeros((5, 3)), None, None, fc), (np.zeros((0, 4)), None, None, fc), (st.astype(complex), None, None, fc),
                (st, np.array([5]), None, fc), (st, np.array([-1]), None, fc), (st, np.zeros(0, np.uint32), None, fc), (st, np.array([0.5]), None, fc),
                (st, None, (1, 0, 0), fc), (st, None, (1, 0, 0, float("nan")), fc), (st, None, (1, 0, 0, float("inf")), fc), (st, None, None, "cfg")):
        with pytest.raises(ValueError):
            o.filter_move(*bad)
    for args in ((None, 5, 1, 5, fc, 1, 1, 1), (1, 5, None, 5, fc, 1, 1, 1), (1, 5, 1, 5, fc, None, 1, 1), (1, 5, 1, 5, fc, 1, None, 1),
                 (1, 5, 1, 5, fc, 1, 1, None), (1, 0, 1, 5, fc, 1, 1, 1), (1, 5, 1, (1 << 22) + 1, fc, 1, 1, 1), (1, 5, 1, 5, "cfg", 1, 1, 1)):
        with pytest.raises(ValueError):
            o.filter_resample_device(*args)
    for args in ((None, 5, 1, 5, None, fc, 1), (1, 5, 1, 5, None, fc, None), (1, 5, None, 6, None, fc, 1), (1, 0, 1, 5, None, fc, 1),
                 (1, 5, 1, 5, (1, 2), fc, 1), (1, 5, 1, 5, None, dict(n_table=0), 1)):
        with pytest.raises(ValueError):
            o.filter_move_device(*args)


def test_the_facades_have_the_filter_step():
    assert callable(radar.RadarHIP.filterStep) and callable(radar.RadarHIP.effectiveSampleSize)
    assert "n_eff_floor" in radar.RadarHIP.filterStep.__doc__ and "never branches" in radar.RadarHIP.filterStep.__doc__
    s = np.zeros(1, native.FILTER_SUMMARY_DTYPE)[0]
    assert radar.RadarHIP.effectiveSampleSize(s) == 0.0
    s["total_weight"], s["sum_w2"] = 12, 48
    assert radar.RadarHIP.effectiveSampleSize(s) == 3.0
    hpp = open(os.path.join(ROOT, "include", "radarays_ros_amd", "RadarHIP.hpp")).read()
    for n in ("filterStep", "rr_filter_config", "rr_filter_summary", "n_eff_floor"):
        assert n in hpp, n
    marshal = open(os.path.join(ROOT, "include", "radarays_ros_amd", "marshal.hpp")).read()
    for n in ("rr_score_poses_device", "rr_filter_resample_device", "rr_filter_move_device"):
        assert n in marshal, n


def test_the_cpp_method_compiles():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "filter_check.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- kernels ------------------------------------------------------------------------------------------------------------------------------
def test_filter_kernels_use_no_scratch(native_lib):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-filter"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    rows, cur = {}, None
    for line in (r.stdout + r.stderr).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        for key, name in ((r"ScratchSize \[bytes/lane\]", "scratch"), (r"LDS Size \[bytes/block\]", "lds"), (r"VGPRs", "vgprs")):
            m = re.search(r"remark:\s+" + key + r": (\d+)", line)
            if m and cur is not None:
                cur[name] = int(m.group(1))
    names = " ".join(rows)
    for k in ("k_flt_init", "k_flt_min", "k_flt_tile", "k_flt_tiles", "k_flt_cum", "k_flt_draw", "k_flt_move"):
        assert k in names, (k, sorted(rows))
    for name, u in rows.items():
        assert u["scratch"] == 0, (name, u)
        assert u["lds"] <= 8192 and u["vgprs"] <= 64, (name, u)                          # eight waves per SIMD


def test_filter_source_is_in_the_library_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rr_filter.hip" in src
    assert re.search(r"^resource-usage-filter:", mk, re.M)
    launch = open(os.path.join(CSRC, "rr_launch.h")).read()
    for name in ("filter_tile_sizes", "launch_filter_resample", "launch_filter_move"):
        assert len(re.findall(r"\b%s\(" % name, launch)) == 1, name
    images = open(os.path.join(CSRC, "rr_images.hip")).read()
    for n in NEW:
        assert re.search(r"^(int|void) %s\(" % n, images, re.M), n
    kernels = open(os.path.join(CSRC, "rr_filter.hip")).read()
    assert "while (" in kernels and kernels.count("while (") == 1                        # the binary search, and no loop that waits
    assert "volatile" not in kernels and "__threadfence" not in kernels                  # no kernel waits on another workgroup
    assert "atomicAdd(float" not in kernels


# ---- the closed loop, on the oracle's images ----------------------------------------------------------------------------------------------
def test_closed_loop_on_the_oracles_images():
    from test_field_host import loop_clouds
    a, b = loop_clouds()
    cfg = F.loop_field_cfg()
    fld = F.distance_field(F.rasterize([a], cfg, F.loop_map_state()), cfg)
    states, xyz = F.loop_lattice()
    rec = F.score(b, states, fld, cfg)
    node = int(np.argmin(rec["sum_d2"]))
    fc = native.filter_config(R.LOOP_SIGMA_XY, R.LOOP_SIGMA_YAW, R.LOOP_QUANTUM, R.LOOP_N_TABLE)
    table = native.filter_weight_table(R.LOOP_SIGMA_CELLS, R.LOOP_QUANTUM, R.LOOP_N_TABLE)
    st = R.loop_particles()
    assert len(st) == 4096
    for k in range(R.LOOP_STEPS):
        recs, cum, anc, s, st = R.step(lambda x: F.score(b, x, fld, cfg), st, table, R.LOOP_QUANTUM, R.loop_phase(k), (1, 0, 0, 0), fc.sigma_xy,
                                       fc.sigma_t, R.LOOP_SEED, k)
        print("step %d: min sum_d2 %d, %d distinct ancestors, n_eff %.0f" % (k, int(s["min_sum_d2"]), int(s["n_unique"]),
                                                                          radar.RadarHIP.effectiveSampleSize(s)))
    recs = F.score(b, st, fld, cfg)
    best = int(np.argmin(recs["sum_d2"]))
    ex, ey, eyaw = R.loop_bound(st[best], recs[best], xyz[node], rec["sum_d2"][node])
    print("closed loop on the oracle's images: §23's node (%.2f m, %.2f m, %.1f deg) at sum_d2 %d; after %d steps the best particle is "
          "(%.3f m, %.3f m, %.2f deg) at sum_d2 %d: %.3f m, %.3f m, %.2f deg from the node"
          % (xyz[node][0], xyz[node][1], math.degrees(xyz[node][2]), rec["sum_d2"][node], R.LOOP_STEPS, st[best][2], st[best][3],
             math.degrees(math.atan2(st[best][1], st[best][0])), recs["sum_d2"][best], ex, ey, math.degrees(eyaw)))
