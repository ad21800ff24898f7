"""Dynamic scenes without a GPU: the new entry points are declared and exported, the Python wrappers refuse bad shapes
before any call into the library, the refit kernels use no scratch, and the vehicle scene helper is deterministic."""
import os
import re
import subprocess

import numpy as np
import pytest

from radarays_ros_amd import native, radar, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radarays_ros_amd", "csrc")


def test_dynamic_entry_points_are_declared_and_exported(native_lib):
    header = open(os.path.join(ROOT, "include", "radarays_mi355.h")).read()
    assert "RR_ABI_VERSION 7" in header


def _unopened(cls):
    """a wrapper object with no library handle: any call that got past the checks would fail differently"""
    o = cls.__new__(cls)
    o._h = None
    o._L = None
    return o


@pytest.mark.parametrize("cls", [native.Context, native.MultiContext])
def test_wrappers_refuse_bad_shapes_before_the_library(cls):
    o = _unopened(cls)
    for bad in (np.zeros((2, 6), np.float32), np.zeros((2, 7, 1), np.float32), np.zeros(8, np.float32),
                np.array([["a"] * 7]), np.zeros((1, 7), np.complex64)):
        with pytest.raises(ValueError):
            o.set_object_poses(bad)
    for bad in (np.zeros((4, 2), np.float32), np.zeros(7, np.float32), np.zeros((2, 3, 3), np.float32)):
        with pytest.raises(ValueError):
            o.update_vertices(bad)
    for bad in ("sah", 2, -1, None):
        with pytest.raises(ValueError):
            o.rebuild_tree(bad)


@pytest.mark.parametrize("cls", [native.Context, native.MultiContext])
def test_set_mesh_refuses_a_face_object_id_of_the_wrong_length_before_the_library(cls):
    """one setter under both classes: the library reads one id per face, so a shorter array would be read past its end"""
    o = _unopened(cls)
    verts, faces = np.zeros((4, 3), np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    for bad in ([0], [0, 1, 1], np.zeros(0, np.uint32)):
        with pytest.raises(ValueError, match="face_object_id must have one entry per face"):
            o.set_mesh(verts, faces, bad)
    assert cls.set_mesh is native.Context.set_mesh


def test_radar_facade_has_the_dynamic_calls():
    for n in ("setObjectPoses", "updateVertices", "rebuildTree", "treeCost"):
        assert callable(getattr(radar.RadarHIP, n)), n


def test_pose_and_vertex_arrays_keep_their_values():
    p = native.object_poses_array([[0, 0, 0, 1, 1, 2, 3]])
    assert p.dtype == np.float32 and p.shape == (1, 7) and p.flags.c_contiguous
    v = native.vertex_array(np.arange(12, dtype=np.float64))
    assert v.shape == (4, 3) and v[3, 2] == 11.0


@pytest.fixture(scope="module")
def refit_usage():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    r = subprocess.run(["make", "-s", "-C", CSRC, "resource-usage-refit"], capture_output=True, text=True, timeout=600)
    rows, cur = {}, None
    for line in (r.stdout + r.stderr).splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        for key, name in ((r"ScratchSize \[bytes/lane\]", "scratch"), ("VGPRs", "vgpr"), (r"Occupancy \[waves/SIMD\]", "occupancy")):
            m = re.search(r"remark:\s+" + key + r": (\d+)", line)
            if m and cur is not None:
                cur[name] = int(m.group(1))
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    return rows


def test_refit_kernels_use_no_scratch(refit_usage):
    names = " ".join(refit_usage)
    for k in ("k_refit_extent", "k_refit_tris", "k_refit_level", "k_tree_cost", "k_gather_refs", "k_pose_soup"):
        assert k in names, (k, sorted(refit_usage))
    for name, u in refit_usage.items():
        assert u["scratch"] == 0 and u["occupancy"] == 8, (name, u)


def test_refit_source_is_in_the_library_build():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", mk, re.M).group(1).split()
    assert "rr_refit.hip" in src


def test_vehicle_helper_is_deterministic_and_keeps_the_scene_as_a_prefix():
    base = scenes.config_scene(2)
    before = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    a = scenes.add_vehicles(base, 64)
    b = scenes.add_vehicles(base, 64)
    for k in ("verts", "faces", "face_object_id", "vehicle_centers"):
        assert np.array_equal(a[k], b[k]), k
    assert a["object_materials"] == b["object_materials"]
    # the original scene is untouched, and is a prefix of the new one
    for k, v in before.items():
        assert (np.array_equal(v, base[k]) if isinstance(v, np.ndarray) else v == base[k]), k
    nv, nf = len(base["verts"]), len(base["faces"])
    assert np.array_equal(a["verts"][:nv], base["verts"]) and np.array_equal(a["faces"][:nf], base["faces"])
    assert np.array_equal(a["face_object_id"][:nf], base["face_object_id"])
    assert len(a["faces"]) == nf + 64 * 12 and len(a["verts"]) == nv + 64 * 8
    first = int(base["face_object_id"].max()) + 1
    assert a["vehicle_objects"] == list(range(first, first + 64))
    assert np.array_equal(a["face_object_id"][nf:], np.repeat(np.arange(first, first + 64), 12))
    assert len(a["object_materials"]) == first + 64 and a["object_materials"][:len(base["object_materials"])] == base["object_materials"]
    assert a["faces"].max() < len(a["verts"]) and a["faces"].dtype == np.uint32 and a["verts"].dtype == np.float32
    # another seed puts them elsewhere
    c = scenes.add_vehicles(base, 64, seed=18)
    assert not np.array_equal(a["verts"], c["verts"])
    # objects without a material table (the ORU4 stand-in) keep none
    o = scenes.add_vehicles(scenes.oru4_like_scene(), 2)
    assert "object_materials" not in o and o["vehicle_objects"] == [18, 19]
