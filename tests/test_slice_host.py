"""Mesh maps without a GPU: the numpy restatement (tests/slice_ref.py) of rr_slice_mesh's definition covers every triangle of every case
and marks nothing a triangle does not reach, with margins that rounding cannot touch and no exceptions; it gives hand-worked answers at
cell corners, borders and band edges; the header, the build and the documents name what was added and the ABI version has not moved; the
wrappers refuse bad arguments before any call into the library; the kernels of rr_slice.hip use no scratch; and the closed loop's figure
is measured on the oracle's image."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import field_ref as F
import slice_ref as R
from radarays_ros_amd import native, params, radar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radarays_ros_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "radarays_mi355.h")
NEW = ["rr_slice_mesh_device", "rr_slice_mesh", "rr_slice_tile_sizes"]


@pytest.fixture(scope="module")
def cases():
    return R.all_cases(*native.slice_tile_sizes())


@pytest.fixture(scope="module")
def maps(cases):
    """the restatement's map of every case, computed once"""
    return [R.slice_mesh(c["soup"], c["obj"], c["skip"], c["band"], c["grid"]) for c in cases]


# ---- 1. the restatement against the geometry ----------------------------------------------------------------------------------------------
def test_the_case_list_is_the_gpu_tests_own_and_reaches_both_kernels(cases):
    small, tile, group = native.slice_tile_sizes()
    labels = [c["label"] for c in cases]
    assert len(labels) == len(set(labels))
    src = open(os.path.join(ROOT, "tests", "test_gpu_slice.py")).read()
    assert "R.all_cases(" in src
    boxes = {c["label"]: R.box_cells(c) for c in cases}
    for n in (small - 1, small, small + 1):
        (label,) = [x for x in labels if x[:2] == ("box", n)]
        assert boxes[label] == [n], (label, boxes[label])
    assert all(b == [257 * 130] for x, b in boxes.items() if x[0] == "diagonal")                   # the whole odd grid: the prefilter's worst case
    (long_label,) = [x for x in labels if x[0] == "long"]
    assert sum(1 for b in boxes[long_label] if b > small) > 256                                    # more list entries than large-kernel groups
    assert max(boxes[("records", 4000)]) <= small                                                  # ... and a case of the small path alone
    for W, H in ((1, 1), (1, 37), (37, 1), (tile - 1, tile + 1), (tile, tile), (tile + 1, tile - 1), (257, 130)):
        assert ("grid", W, H) in labels
    for n in (1, group - 1, group, group + 1, 4000):
        assert ("records", n) in labels


def test_covering_and_tightness_hold_on_every_case_without_exception(cases, maps):
    """m = 1/256 cell and m_z = 1e-4 m: about 16 f32 ulps at 4096 cells and 64 m.  Every f64 sample of a triangle that far inside a cell
    and the band sits in a marked cell; every marked cell is reached by a triangle in f64 once grown by the same margins"""
    assert R.M_CELL == 1.0 / 256.0 and R.M_Z == 1e-4
    checked = marked = n_cases = 0
    for c, (occ, _) in zip(cases, maps):
        if not R.in_range(c):
            assert c["label"][0] == "single" and "1e30" in c["label"][1], c["label"]
            continue
        n, missed = R.covering(occ, c)
        m, loose = R.tightness(occ, c)
        assert missed == 0, (c["label"], n, missed)
        assert loose == 0, (c["label"], m, loose)
        checked, marked, n_cases = checked + n, marked + m, n_cases + 1
    print("covering: %d samples, tightness: %d marked cells, over %d cases" % (checked, marked, n_cases))
    assert checked > 100000 and marked > 10000 and n_cases >= 50


def test_a_predicate_without_an_axis_or_with_a_shrunk_box_is_caught(cases, maps, monkeypatch):
    """the two checks are sharp enough to tell: without the (0,0,1) x e axes a thin diagonal triangle marks its whole bounding box
    (tightness), and a cell box of half the side loses cells that samples sit in (covering)"""
    k = [c["label"] for c in cases].index(("diagonal", "level", "plain"))
    c = cases[k]
    keep = R._sat
    monkeypatch.setattr(R, "_sat", lambda u, v, z, cu, cv, cz, hu, hv, hz: np.ones(np.broadcast(cu, cv).shape, bool))
    loose, _ = R.slice_mesh(c["soup"], c["obj"], None, c["band"], c["grid"])
    monkeypatch.setattr(R, "_sat", keep)
    assert loose.sum() == 257 * 130 and R.covering(loose, c)[1] == 0 and R.tightness(loose, c)[1] > 30000
    k = [c["label"][0] for c in cases].index("long")
    c = cases[k]
    monkeypatch.setattr(R, "_sat", lambda u, v, z, cu, cv, cz, hu, hv, hz: keep(u, v, z, cu, cv, cz, hu * R.F32(0.5), hv * R.F32(0.5), hz))
    thin, _ = R.slice_mesh(c["soup"], c["obj"], None, c["band"], c["grid"])
    assert thin.sum() < maps[k][0].sum() and R.covering(thin, c)[1] > 0


def test_hand_worked_cells(cases, maps):
    by = {c["label"]: occ for c, (occ, _) in zip(cases, maps)}
    cell = lambda occ: sorted(zip(*[a.tolist() for a in np.nonzero(occ)[::-1]]))      # noqa: E731  (ix, iy) pairs
    assert cell(by[("single", "a point inside a cell")]) == [(5, 5)]
    assert cell(by[("single", "a point on a cell corner")]) == [(4, 4), (4, 5), (5, 4), (5, 5)]             # touching counts, on all four sides
    assert cell(by[("single", "touching the grid's high corner from outside")]) == [(23, 19)]
    border = by[("single", "an edge along a cell border")]
    assert border[2, 3:10].all() and border[3, 3:10].all() and not border[1].any()                          # both sides of the border v = 3
    assert border[2, 3] and not border[2, 2]                                                                # ... from the cell left of the corner u = 4
    for name in ("one ulp below the band", "one ulp above the band", "top one ulp below z_lo", "a plane band, horizontal one ulp off", "outside, low u",
                 "outside, high u", "outside, low v", "outside, high v"):
        assert not by[("single", name)].any(), name
    assert np.array_equal(by[("single", "horizontal on z_lo")], by[("single", "horizontal, inside the band")])
    assert np.array_equal(by[("single", "horizontal on z_hi")], by[("single", "a plane band, horizontal in it")])
    assert by[("single", "top exactly on z_lo")].sum() == 1 and by[("single", "bottom exactly on z_hi")].sum() == 1
    assert by[("single", "over the whole grid and beyond")].all()
    diag = by[("single", "collinear through cell corners")]
    assert all(diag[k, k] for k in range(1, 11)) and diag.sum() == 28                                        # the diagonal and both neighbours
    wall = by[("single", "wall with no area in xy")]
    # the band cuts the wall between a quarter of the way up its sloping edge, at (4.325, 5.4), and its vertical edge at (7.7, 9.3)
    assert wall.sum() == 8 and wall[5, 4] and wall[9, 7] and not wall[4, 3]


def test_object_plane_skip_list_and_accumulation_of_the_restatement():
    g = R.grid(12, 10)
    soup = R.xyz([[[1.5, 1.5, 0.5], [6.5, 1.5, 0.5], [1.5, 6.5, 0.5]], [[3.5, 3.5, 0.2], [9.5, 3.5, 0.2], [3.5, 8.5, 0.2]],
                  [[2.5, 2.5, 2.5], [7.5, 2.5, 2.5], [2.5, 7.5, 2.5]]], g)
    obj = np.array([5, 2, 0], np.uint32)
    occ, ids = R.slice_mesh(soup, obj, None, (0.0, 1.0), g)
    assert set(np.unique(ids)) == {2, 5, R.OBJECT_NONE} and np.array_equal(ids != R.OBJECT_NONE, occ == 1)
    assert ids[4, 4] == 2 and ids[1, 1] == 5                                                                 # the minimum where two overlap
    skip = np.array([0, 0, 1, 0, 0, 0], np.uint8)
    only5, _ = R.slice_mesh(soup, obj, skip, (0.0, 1.0), g)
    assert np.array_equal(only5, R.slice_mesh(soup[:1], obj[:1], None, (0.0, 1.0), g)[0])
    upper, _ = R.slice_mesh(soup, obj, None, (2.0, 3.0), g)
    both, _ = R.slice_mesh(soup, obj, None, (2.0, 3.0), g, occ=occ)
    assert np.array_equal(both, occ | upper) and upper.any() and not np.array_equal(both, occ)
    pre = np.zeros((10, 12), np.uint8)
    pre[9, 11] = 200
    assert R.slice_mesh(soup, obj, None, (0.0, 1.0), g, occ=pre)[0][9, 11] == 200                            # nothing is cleared


# ---- 2. headers, build, documents -----------------------------------------------------------------------------------------------------------
def test_slice_entry_points_are_declared_and_exported(native_lib):
    header = open(HEADER).read()
    assert "#define RR_ABI_VERSION 7" in header
    L = native_lib.lib()
    assert L.rr_abi_version() == 7
    for n in NEW:
        assert n in native.SYMBOLS and hasattr(L, n) and re.search(r"\b%s\(" % n, header), n
    small, tile, group = native_lib.slice_tile_sizes()
    assert small >= 1 and tile >= 2 and tile * tile == 64 and group % 64 == 0
    assert C.sizeof(native.RRSliceConfig) == 16 and re.search(r"typedef struct rr_slice_config \{\s*/\* 16 B \*/", header)
    assert "rr_slice_config" in native.STRUCTS
    for word in ("CELL PREDICATE", "CANDIDATE CELLS", "UNPINNED", "rr_rebuild_tree", "tests/slice_ref.py"):
        assert word in header[header.index("mesh maps: the scene's triangles"):header.index("several GPUs of one node")], word


def test_slice_config_is_range_checked():
    s = native.slice_config(-0.5, 1.25)
    assert (s.z_lo, s.z_hi, s.flags, s.reserved_) == (-0.5, 1.25, 0, 0)
    assert native.slice_config(0.5, 0.5).z_lo == 0.5
    for bad in ((1.0, 0.5), (float("nan"), 1.0), (0.0, float("inf")), (-1e39, 0.0), ("low", 1.0), (True, 2.0)):
        with pytest.raises(ValueError):
            native.slice_config(*bad)
    with pytest.raises(ValueError):
        native._slice_cfg(native.RRSliceConfig(0.0, 1.0, 1, 0))
    with pytest.raises(ValueError):
        native._slice_cfg({"z_lo": 0.0})
    assert native._slice_cfg((0.0, 1.0)).z_hi == 1.0


def test_wrappers_refuse_bad_arguments_before_the_library():
    o = native.Context.__new__(native.Context)
    o._h = o._L = None
    o.n_objects = 3
    g = native.field_config(8, 6, 0.5, 0.0, 0.0, 4, 1)
    for kw in (dict(occ=np.zeros((6, 8), np.uint16)), dict(occ=np.zeros((8, 6), np.uint8)), dict(objects=np.zeros((6, 8), np.int32)),
               dict(skip_objects=[3]), dict(skip_objects=[-1]), dict(skip_objects=[0.5])):
        with pytest.raises(ValueError):
            o.slice_mesh((0.0, 1.0), g, **kw)
    for args in (((1.0, 0.0), g, 1), ((0.0, 1.0), "grid", 1), ((0.0, 1.0), g, None), ((0.0, 1.0), g, 1, 6)):
        with pytest.raises(ValueError):
            o.slice_mesh_device(*args)
    assert list(o._skip_bytes([2, 0])) == [1, 0, 1] and o._skip_bytes(()) is None and o._skip_bytes(None) is None


def test_the_facades_have_the_mesh_map():
    assert callable(radar.RadarHIP.buildMeshMap)
    doc = radar.RadarHIP.buildMeshMap.__doc__
    for word in ("buildLikelihoodField", "buildNearestField", "scoreBeams", "skip_objects"):
        assert word in doc, word
    hpp = open(os.path.join(ROOT, "include", "radarays_ros_amd", "RadarHIP.hpp")).read()
    for n in ("buildMeshMap", "rr_slice_config", "rr_slice_mesh"):
        assert n in hpp, n


def test_the_cpp_driver_compiles():
    src = os.path.join(ROOT, "tests", "cpp", "slice_check.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), src],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "buildMeshMap" in open(src).read()


def test_slice_kernels_use_no_scratch(native_lib):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-slice"], capture_output=True, text=True, timeout=600)
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
    for kname in ("k_slice_small", "k_slice_large"):
        assert kname in names, (kname, sorted(rows))
    assert len(rows) == 2
    for name, u in rows.items():
        assert u["scratch"] == 0, (name, u)
        assert u["lds"] == 0, (name, u)
        assert u["vgprs"] <= 96, (name, u)                             # at least five waves per SIMD (DESIGN.md §28 states the counts)


def test_slice_source_is_in_the_library_build_and_the_documents():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    hdr = re.search(r"^HDR\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rr_slice.hip" in src and "rr_posed.h" in hdr
    assert re.search(r"^resource-usage-slice:", mk, re.M)
    launch = open(os.path.join(CSRC, "rr_launch.h")).read()
    for name in ("slice_tile_sizes", "slice_scratch_words", "launch_slice"):
        assert len(re.findall(r"\b%s\(" % name, launch)) == 1, name
    images = open(os.path.join(CSRC, "rr_images.hip")).read()
    for n in NEW:
        assert re.search(r"^(int|void) %s\(" % n, images, re.M), n
    # posed_face lives in ONE header, which both users include; the cell rule's helper lives in rr_grid.h
    refit, kernels = open(os.path.join(CSRC, "rr_refit.hip")).read(), open(os.path.join(CSRC, "rr_slice.hip")).read()
    posed = open(os.path.join(CSRC, "rr_posed.h")).read()
    assert len(re.findall(r"inline void posed_face\(", posed)) == 1 and "inline void posed_face(" not in refit + kernels
    assert '#include "rr_posed.h"' in refit and '#include "rr_posed.h"' in kernels
    assert "cell_coord(" in open(os.path.join(CSRC, "rr_grid.h")).read() and "cell_coord(" in kernels
    assert "__shared__" not in kernels and "__syncthreads" not in kernels and kernels.count("__global__") == 2
    readme, design, baseline = (open(os.path.join(ROOT, f)).read() for f in ("README.md", "DESIGN.md", "BASELINE.md"))
    assert "rr_slice.hip" in readme and "rr_slice_mesh" in readme
    assert re.search(r"^## 28\.", design, re.M) and "k_slice_small" in design and "k_slice_large" in design and "UNPINNED" in design
    assert re.search(r"^## 25\.", baseline, re.M) and "probe_slice.py" in baseline
    assert os.path.exists(os.path.join(ROOT, "tools", "probe_slice.py"))


# ---- 3. the closed loop's figure, measured here on the oracle's image ---------------------------------------------------------------------
def test_closed_loop_figure_on_the_oracles_image():
    """the scan detected on the oracle's image of the box room at pose B, scored over field_ref's lattice (steps of 0.25 m and 1 degree) against
    the distance field of the restatement's map of the room's mesh, sliced at the sensor's height"""
    from test_field_host import loop_clouds
    _, b = loop_clouds()
    cfg = F.loop_field_cfg()
    soup, obj = R.loop_soup()
    occ, _ = R.slice_mesh(soup, obj, None, R.LOOP_BAND, cfg)
    fld = F.distance_field(occ, cfg)
    states, xyz = F.loop_lattice()
    rec = F.score(b, states, fld, cfg)
    best, centre = int(np.argmin(rec["sum_d2"])), len(states) // 2
    ex, ey, eyaw = F.loop_errors(xyz[best])
    print("closed loop on the oracle's image: %d cells occupied; argmin node (%.2f m, %.2f m, %.1f deg) at sum_d2 %d (centre node %d), off the "
          "truth by %.3f m, %.3f m, %.3f deg; lattice steps %.2f m, %.1f deg"
          % (occ.sum(), xyz[best][0], xyz[best][1], math.degrees(xyz[best][2]), rec["sum_d2"][best], rec["sum_d2"][centre], ex, ey,
             math.degrees(eyaw), F.LOOP_STEP_XY, math.degrees(F.LOOP_STEP_YAW)))
    assert np.count_nonzero(rec["sum_d2"] == rec["sum_d2"][best]) == 1 and rec["sum_d2"][best] < rec["sum_d2"][centre]
    assert np.all(rec["n_in"] == len(b))
    assert (F.LOOP_STEP_XY, round(math.degrees(F.LOOP_STEP_YAW), 9)) == (0.25, 1.0)
    assert ex <= F.LOOP_STEP_XY and ey <= F.LOOP_STEP_XY and eyaw <= F.LOOP_STEP_YAW
    # the constants are what is measured here
    assert abs(ex - R.LOOP_X_MEASURED) <= 1e-9 and abs(ey - R.LOOP_Y_MEASURED) <= 1e-9 and abs(eyaw - R.LOOP_YAW_MEASURED) <= 1e-9
