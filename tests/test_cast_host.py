"""The beam model without a GPU: the skip rule of k_cast as tests/cast_ref.py restates it equals the brute-force march, element for element, on
every case of the GPU tests and on seeded random states of three scales; the classification keeps its identities; the header, the build and
the documents name what was added; the kernels of rr_cast.hip use no scratch; and the closed loop's figures are measured on the oracle's
images."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cast_ref as R
import field_ref as F
import icp_ref
import occupancy_ref as O
from radarays_ros_amd import native, radar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radarays_ros_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "radarays_mi355.h")
NEW = ["rr_scan_profile_device", "rr_scan_profile", "rr_cast_map_device", "rr_cast_map", "rr_score_beams_device", "rr_score_beams",
       "rr_cast_tile_sizes"]


# ---- 1. the skip rule against the definition -------------------------------------------------------------------------------------------------
def _march(c):
    """one case of cast_ref's list: skip_march against brute, element for element -> the bins the skip saved on rays that met nothing"""
    want = R.case_brute(c)
    got, looks, visits = R.case_skip(c)
    assert np.array_equal(got, want), (c["label"], np.argwhere(got != want)[:4])
    beam = c["beam"]
    bins = len(range(beam.bin_begin, beam.bin_end, beam.bin_step))
    assert np.all(looks <= visits) and np.all(visits <= bins)
    return int((bins - visits)[want == beam.bin_end].sum())


def _host_cases():
    return list(R.host_cases(*native.cast_tile_sizes()[1:]))


def test_the_case_list_is_the_gpu_tests_own():
    """tests/test_gpu_cast.py iterates the same generators: full_cases, azimuth_cases, records_case, small_case, stream_case"""
    labels = [c["label"] for c in _host_cases()]
    assert len(labels) == len(set(labels))
    assert sum(1 for x in labels if x[0] == "full") == len(R.GRIDS) * len(R.BIN_STEPS)
    per_A = len(R.AZIMUTH_MAPS) * len(R.BIN_STEPS) * len(R.WINDOWS)
    for A in R.ANGLES:
        assert sum(1 for x in labels if x[0] == A) == (0 if A == R.FULL_ANGLES else per_A), A
    for name in ("records", "records, empty window", "host forms", "two streams"):
        assert (name,) in labels
    src = open(os.path.join(ROOT, "tests", "test_gpu_cast.py")).read()
    for gen in ("R.full_cases(", "R.azimuth_cases(", "R.records_case(", "R.small_case(", "R.stream_case("):
        assert gen in src, gen


@pytest.mark.parametrize("k", range(len(R.GRIDS)))
def test_skip_march_equals_brute_force_on_every_map_saturation_and_bin_step(k):
    skipped = sum(_march(dict(c, label=("full", k, c["step"]))) for c in R.full_cases(k)[2])
    assert skipped > 0                                                # the rule does skip: a ray that meets nothing visits fewer bins than there are


@pytest.mark.parametrize("A", [a for a in R.ANGLES if a != R.FULL_ANGLES])
def test_skip_march_equals_brute_force_at_every_azimuth_count(A):
    for c in R.azimuth_cases(A):
        _march(c)


def test_skip_march_equals_brute_force_on_the_records_host_form_and_stream_cases():
    rest = [c for c in _host_cases() if isinstance(c["label"][0], str) and c["label"][0] != "full"]
    assert len(rest) == 4
    for c in rest:
        _march(c)


@pytest.mark.parametrize("k", range(len(R.GRIDS)))
def test_skip_march_equals_brute_force_on_random_states(k):
    """2,000 seeded states per map, |(c, s)| of 0.5, 1 and 2, the direction table scaled likewise"""
    W, H, cell, res = R.GRIDS[k]
    rs = np.random.RandomState(900 + k)
    for name, occ in R.map_list(W, H).items():
        md = R.SATURATIONS[rs.randint(len(R.SATURATIONS))]
        cfg = R.grid_cfg(k, md)
        fld = F.distance_field(occ, cfg)
        n = 2000
        yaw = rs.uniform(-np.pi, np.pi, n)
        norm = np.array([0.5, 1.0, 2.0])[rs.randint(3, size=n)]
        tx = rs.uniform(R.X0 - 2 * cell, R.X0 + (W + 2) * cell, n)
        ty = rs.uniform(R.Y0 - 2 * cell, R.Y0 + (H + 2) * cell, n)
        sts = np.stack([norm * np.cos(yaw), norm * np.sin(yaw), tx, ty], axis=1).astype(np.float32)
        for scale, step in ((1.0, 1), (0.5, 1), (2.0, 3)):
            dirs = R.dir_table(5, scale, theta_min=float(rs.uniform(0, 1)))
            beam = R.beam(step)
            want = R.brute(sts, dirs, fld, cfg, beam, res)
            got, _, _ = R.skip_march(sts, dirs, fld, cfg, beam, res)
            assert np.array_equal(got, want), (k, name, md, scale, step, np.argwhere(got != want)[:4])


def test_a_rule_without_its_margin_is_caught():
    """the comparison is sharp enough to tell: with the two half diagonals of a cell left out of the rule, rays slip through walls"""
    k = 1
    res = R.GRIDS[k][3]
    cfg = R.grid_cfg(k, 16)
    occ = R.map_list(*R.GRIDS[k][:2])["diagonal"]
    fld = F.distance_field(occ, cfg)
    sts, dirs, beam = R.state_list(cfg, occ), R.dir_table(400), R.beam(1)
    want = R.brute(sts, dirs, fld, cfg, beam, res)
    assert np.array_equal(R.skip_march(sts, dirs, fld, cfg, beam, res)[0], want)
    keep = R.DIAG
    try:
        R.DIAG = np.float32(-1.0)
        assert not np.array_equal(R.skip_march(sts, dirs, fld, cfg, beam, res)[0], want)
    finally:
        R.DIAG = keep


# ---- 2. classification -------------------------------------------------------------------------------------------------------------------------
def test_classification_identities():
    rs = np.random.RandomState(11)
    A, n, n_cells = 129, 300, R.N_CELLS
    for begin, end, tol, clip in ((0, n_cells, 0, 0), (10, 200, 6, 24), (10, 200, n_cells, 5), (31, 31, 3, 3), (0, 1, 1, n_cells)):
        beam = native.beam_config(begin, end, n_cells, 1, tol, clip)
        e = np.where(rs.random_sample((n, A)) < 0.3, end, rs.randint(begin, max(end, begin + 1), (n, A))).clip(begin, end)
        m = rs.randint(0, n_cells + 1, A)
        rec = R.classify(e, m, beam)
        assert np.all(rec["n_agree"] + rec["n_short"] + rec["n_through"] + rec["n_open"] + rec["n_none"] == rec["n_cast"])
        assert np.all(rec["n_cast"] == (m >= begin).sum())
        assert np.all(rec["sum_abs"] <= clip * (rec["n_agree"] + rec["n_short"] + rec["n_through"]).astype(np.int64))
        if begin == end:                                              # nothing is sampled, and every azimuth is "none" on both sides
            assert not (rec["n_agree"].any() or rec["n_short"].any() or rec["n_through"].any() or rec["n_open"].any() or rec["sum_abs"].any())
            assert np.all(rec["n_none"] == rec["n_cast"])
        if tol >= n_cells:
            assert not rec["n_short"].any()
            assert np.array_equal(rec["n_through"], ((e < end) & (m[None, :] >= end) & (m[None, :] >= begin)).sum(axis=1))
    # a hand-worked row: e = 50; m = 43 (short), 44 and 56 (agree at the edge), 57 (through), none (through), below the window (left out)
    beam = native.beam_config(10, 200, n_cells, 1, 6, 9)
    rec = R.classify(np.full((1, 6), 50), np.array([43, 44, 56, 57, 200, 9]), beam)[0]
    assert (rec["n_short"], rec["n_agree"], rec["n_through"], rec["n_open"], rec["n_none"], rec["n_cast"], rec["sum_abs"]) == (1, 2, 2, 0, 0, 5, 7 + 6 + 6 + 7)
    rec = R.classify(np.full((1, 3), 200), np.array([43, 200, 255]), beam)[0]
    assert (rec["n_open"], rec["n_none"], rec["n_cast"], rec["sum_abs"]) == (1, 2, 3, 0)


def test_profile_restatement_on_a_hand_worked_scan():
    """pins the RESTATEMENT to hand-worked values, so that the GPU tests compare rr_scan_profile with something held independently; it runs
    no code of the library"""
    p = np.zeros(5, native.POINT_DTYPE)
    p["column"], p["bin"] = [0, 0, 2, 3, 3], [7, 9, 4, 300, 301]
    offs = np.array([[0, 2, 2, 3, 5]], np.uint32)
    assert list(R.profile([p], offs, 256, 4)[0]) == [7, 256, 4, 256]                     # a bin past n_cells is cut at it
    assert list(R.profile([p], offs, 256, 4, scroll=1)[0]) == [256, 4, 256, 7]            # azimuth a sits in column a + 1
    assert list(R.profile([p], offs, 256, 4, max_points=2)[0]) == [7, 256, 256, 256]      # the first detections of columns 2 and 3 were cut


# ---- 3. headers and build ------------------------------------------------------------------------------------------------------------------------
def test_cast_entry_points_are_declared_and_exported(native_lib):
    header = open(HEADER).read()
    assert "#define RR_ABI_VERSION 7" in header
    L = native_lib.lib()
    assert L.rr_abi_version() == 7
    for n in NEW:
        assert n in native.SYMBOLS and hasattr(L, n) and re.search(r"\b%s\(" % n, header), n
    angles_tile, per_wave, per_group = native_lib.cast_tile_sizes()
    assert angles_tile == 64 and per_wave >= 1 and per_group >= per_wave and per_group % per_wave == 0
    assert native.BEAM_DTYPE.itemsize == 32
    import ctypes as C
    assert C.sizeof(native.RRBeamConfig) == 32 and C.sizeof(native.RRBeamRec) == 32
    assert re.search(r"typedef struct rr_beam_config \{\s*/\* 32 B \*/", header) and re.search(r"typedef struct rr_beam_rec \{\s*/\* 32 B \*/", header)


def test_beam_config_and_directions():
    b = native.beam_config(3, 200, 256, 2, 6, 24)
    assert (b.bin_begin, b.bin_end, b.bin_step, b.tol_bins, b.clip_bins, list(b.reserved_)) == (3, 200, 2, 6, 24, [0, 0, 0])
    for bad in (dict(bin_begin=-1), dict(bin_begin=201), dict(bin_end=257), dict(bin_step=0), dict(bin_step=65), dict(tol_bins=257), dict(clip_bins=-1),
                dict(n_cells=65536), dict(bin_step=1.5)):
        kw = dict(bin_begin=3, bin_end=200, n_cells=256, bin_step=2, tol_bins=6, clip_bins=24)
        kw.update(bad)
        with pytest.raises(ValueError):
            native.beam_config(**kw)
    rr = native.make_config(icp_ref.loop_cfg(), icp_ref.LOOP_ANGLES)
    d = native.beam_directions(rr)
    assert d.dtype == np.float32 and d.shape == (icp_ref.LOOP_ANGLES, 2)
    theta = float(rr.theta_min) + np.arange(icp_ref.LOOP_ANGLES) * float(rr.theta_inc)
    assert np.array_equal(d[:, 0], np.cos(theta).astype(np.float32)) and np.array_equal(d[:, 1], np.sin(theta).astype(np.float32))


def test_the_facades_have_the_beam_calls():
    for n in ("scanProfile", "castMap", "scoreBeams"):
        assert callable(getattr(radar.RadarHIP, n)), n
    assert "sensor frame into the map frame" in radar.RadarHIP.scoreBeams.__doc__
    hpp = open(os.path.join(ROOT, "include", "radarays_ros_amd", "RadarHIP.hpp")).read()
    for n in ("castMap", "scoreBeams", "rr_beam_rec", "marshal::cast_map", "marshal::score_beams"):
        assert n in hpp, n
    marshal = open(os.path.join(ROOT, "include", "radarays_ros_amd", "marshal.hpp")).read()
    assert "rr_cast_map_device" in marshal and "rr_score_beams_device" in marshal


def test_the_cpp_methods_compile():
    """(syntax only, as refine_check.cpp; the refusal of null buffers is run by tests/test_gpu_cast.py::test_refusals_write_nothing)"""
    src = os.path.join(ROOT, "tests", "cpp", "cast_check.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    text = open(src).read()
    assert "castMap" in text and "scoreBeams" in text and "nullptr" in text


def test_cast_kernels_use_no_scratch(native_lib):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-cast"], capture_output=True, text=True, timeout=600)
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
    for kname in ("k_scan_profile", "k_castILb1E", "k_castILb0E"):
        assert kname in names, (kname, sorted(rows))
    for name, u in rows.items():
        assert u["scratch"] == 0, (name, u)
        assert u["lds"] == 0, (name, u)
        assert u["vgprs"] <= 64, (name, u)                            # eight waves per SIMD


def test_cast_source_is_in_the_library_build_and_the_documents():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rr_cast.hip" in src
    assert re.search(r"^resource-usage-cast:", mk, re.M)
    launch = open(os.path.join(CSRC, "rr_launch.h")).read()
    for name in ("cast_tile_sizes", "launch_scan_profile", "launch_cast"):
        assert len(re.findall(r"\b%s\(" % name, launch)) == 1, name
    images = open(os.path.join(CSRC, "rr_images.hip")).read()
    for n in NEW:
        assert re.search(r"^(int|void) %s\(" % n, images, re.M), n
    kernels = open(os.path.join(CSRC, "rr_cast.hip")).read().split("namespace rr {", 1)[1]
    assert "atomic" not in kernels and "__syncthreads" not in kernels and "__shared__" not in kernels
    assert kernels.count("__global__") == 2                           # the profile, and ONE templated body for both ray calls
    readme, design = open(os.path.join(ROOT, "README.md")).read(), open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "rr_cast.hip" in readme
    for n in ("rr_scan_profile", "rr_cast_map", "rr_score_beams"):
        assert n in readme and n in design, n
    assert re.search(r"^## 27\.", design, re.M) or "§27" in design


# ---- 4. the closed loop, on the oracle's images ---------------------------------------------------------------------------------------------------
def test_closed_loop_on_the_oracles_images():
    from test_occupancy_host import loop_clouds
    clean, offs, scan_a, scan_b = loop_clouds()
    G, cfg, st = O.loop_polar(), F.loop_field_cfg(), O.loop_states()
    field_cfg = native.field_config(cfg.width, cfg.height, cfg.cell, cfg.x0, cfg.y0, R.LOOP_MAX_DIST, 0)
    occ_map = O.to_map(O.update(clean, offs, cfg, G, O.LOOP_MODEL, st))
    fld = F.distance_field(occ_map, field_cfg, R.LOOP_THRESHOLD)
    beam = R.loop_beam(G.resolution)
    assert (beam.bin_begin, beam.bin_end, beam.bin_step, beam.tol_bins, beam.clip_bins) == (0, 279, 1, 6, 24)
    dirs = native.beam_directions(native.make_config(icp_ref.loop_cfg(), icp_ref.LOOP_ANGLES))
    A = icp_ref.LOOP_ANGLES

    def offsets_of(cloud):
        o = np.zeros((1, A + 1), np.uint32)
        o[0, 1:] = np.cumsum(np.bincount(cloud["column"].astype(np.int64), minlength=A))
        return o

    prof_a = R.profile([scan_a], offsets_of(scan_a), G.n_cells, A)[0]
    prof_b = R.profile([scan_b], offsets_of(scan_b), G.n_cells, A)[0]
    states, xyz = F.loop_lattice()
    e = R.brute(states, dirs, fld, field_cfg, beam, G.resolution)
    got, looks, visits = R.skip_march(states, dirs, fld, field_cfg, beam, G.resolution)
    assert np.array_equal(got, e)
    recs = R.classify(e, prof_b, beam)
    wall_states = R.loop_behind_wall()
    wall = R.score(prof_a, wall_states, dirs, fld, field_cfg, beam, G.resolution)
    best = R.loop_best(recs)
    brute_bins = np.minimum((e.astype(np.int64) - beam.bin_begin) // beam.bin_step + 1, len(range(beam.bin_begin, beam.bin_end, beam.bin_step)))
    print("closed loop on the oracle's images: argmax node (%.2f m, %.2f m, %.1f deg) %s, the centre node %s; n_through at A %d, behind the wall "
          "%d (%s); look-ups per ray %.2f (samples computed %.2f) where the brute force visits %.2f bins"
          % (xyz[best][0], xyz[best][1], math.degrees(xyz[best][2]), recs[best], recs[len(recs) // 2], wall[0]["n_through"], wall[1]["n_through"],
             wall[1], looks.mean(), visits.mean(), brute_bins.mean()))
    R.loop_check(recs, xyz, wall)
