"""The device-side tree builder (rr_lbvh.hip) at its structural edges: for every case of tests/lbvh_ref.py the tree of
builder="gpu" -- and, to tell a builder's fault from the traversal's, the tree of builder="host" -- must give, ray by ray and
bit by bit, what the oracle's brute-force loop gives (the nearest hit does not depend on the tree).

  1  2 .. 513 congruent, separated triangles: the one-leaf root up to kMaxLeafTris = 4, the first inner child at 5, one and two
     launch blocks of k_karras / k_refit at 256 / 257
  2  300 boxes on one centre and 150 pairs on theirs: delta()'s index tie-break decides whole subtrees, across a block boundary
  3  no extent in z; a 400 m x 0.5 m x 0.5 m strip under the one cubic Morton scale
  4  two faces longer than kMaxCellsPerAxis = 24 cells of the settled size, rays at the planes of every cell size the bisection
     can settle on; the same scene with RR_LBVH_NO_SPLIT=1
  5  case 4 at (+6000, -6000, +500) m, its brute force recomputed
  6  a Morton chain: the one case where k_collapse's stack accounting is deep, at the default and the one-entry LDS stack
  7  faces without area among case 1's 257 triangles (k_split's "numerically empty everywhere: keep it whole")
  8  three builds on one context: atomics' arrival order must not show
  9  what the GPU builder refuses, and what it then leaves in place

There is no tolerance in this file; tests/test_lbvh_host.py holds the references to what keeps these tests from being vacuous."""
import numpy as np
import pytest

import lbvh_ref as B
from common import assert_trace_equals_brute_force, golden_beams
from radarays_ros_amd import params, scenes

pytestmark = pytest.mark.gpu

BUILDERS = ["gpu", "host"]


def _built(native_lib, st, builder):
    c = native_lib.Context(0)
    c.set_mesh(st["verts"], st["faces"], None, builder=builder)
    return c


def _trace_case(native_lib, oracle, name, builder):
    st = B.case(oracle, name)
    c = _built(native_lib, st, builder)
    info = c.bvh_info()
    print(name, builder, info)
    assert_trace_equals_brute_force(c, st, builder, "as built")
    c.close()
    return st, info


# ---- 1. reference counts around the leaf size and the launch block ---------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("n", B.COUNTS)
def test_separated_triangles_equal_brute_force(native_lib, oracle, n, builder):
    _trace_case(native_lib, oracle, "separated:%d" % n, builder)


@pytest.mark.parametrize("n", B.COUNTS)
def test_separated_triangles_unsplit_reach_the_counts_themselves(native_lib, oracle, monkeypatch, n):
    """RR_LBVH_NO_SPLIT=1: the same counts with split clipping off altogether (the bisection does not run)"""
    monkeypatch.setenv("RR_LBVH_NO_SPLIT", "1")
    st, info = _trace_case(native_lib, oracle, "separated:%d" % n, "gpu")
    assert info["n_tris"] == n
    if n <= B.K_MAX_LEAF:
        assert info["n_nodes"] == 1 and info["depth"] == 1, info
    elif n > 16:                                                              # (four leaves of four fill one node)
        assert info["n_nodes"] > 1 and info["depth"] > 1, info


def test_equal_sized_triangles_are_not_cut(native_lib, oracle):
    """Congruent triangles: split clipping has no face "much larger than its neighbours" to cut, so the tree holds n records, and
    up to kMaxLeafTris of them are one leaf of the root.  (Before k_side and the size gate of k_split the builder cut every face
    at every grid plane it straddled and spent its budget here too: n -> n_tris was 2 -> 66, 4 -> 68, 257 -> 382, 513 -> 704.)"""
    got = {}
    for n in B.COUNTS:
        c = _built(native_lib, B.case(oracle, "separated:%d" % n), "gpu")
        got[n] = c.bvh_info()
        c.close()
        print("n", n, got[n])
    for n in B.COUNTS:
        assert got[n]["n_tris"] == n, (n, got[n])
        if n <= B.K_MAX_LEAF:
            assert got[n]["n_nodes"] == 1 and got[n]["depth"] == 1, (n, got[n])


# ---- 2, 3. equal Morton codes in bulk; flat and thin extents ----------------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", ["coincident", "flat", "strip"])
def test_equal_codes_and_thin_extents_equal_brute_force(native_lib, oracle, name, builder):
    _trace_case(native_lib, oracle, name, builder)


# ---- 4, 5. split clipping at its cap, near the origin and far from it -------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("name", ["capped", "capped:far"])
def test_faces_beyond_the_cell_cap_equal_brute_force(native_lib, oracle, name, builder):
    st, info = _trace_case(native_lib, oracle, name, builder)
    nf = len(st["faces"])
    if builder == "gpu":
        assert nf < info["n_tris"] <= nf + nf // 4 + 64, (info, nf)           # it cut, and within its stated budget


@pytest.mark.parametrize("name", ["capped", "capped:far"])
def test_unsplit_build_traces_the_same(native_lib, oracle, monkeypatch, name):
    st = B.case(oracle, name)
    c = _built(native_lib, st, "gpu")
    t0, f0 = assert_trace_equals_brute_force(c, st, "gpu", "split")
    assert c.bvh_info()["n_tris"] > len(st["faces"])
    c.close()
    monkeypatch.setenv("RR_LBVH_NO_SPLIT", "1")
    c = _built(native_lib, st, "gpu")
    assert c.bvh_info()["n_tris"] == len(st["faces"])
    t1, f1 = assert_trace_equals_brute_force(c, st, "gpu", "RR_LBVH_NO_SPLIT=1")
    c.close()
    assert np.array_equal(t0.view(np.uint32), t1.view(np.uint32)) and np.array_equal(f0, f1)


# ---- 6. a Morton chain: depth and the stack bound ---------------------------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
@pytest.mark.parametrize("lds", [None, "1"], ids=["lds-default", "lds-1"])
def test_morton_chain_equals_brute_force(native_lib, oracle, monkeypatch, lds, builder):
    """stack_need is the builder's promise to the traversal: entries beyond it are not kept, so a bound too small drops hits.  The
    LDS stack a context uses is min(stack_need, 64, RR_STACK_LDS); with RR_STACK_LDS=1 every entry but one lies in the spill
    buffer, which is sized by stack_need.  The chain peels one position (a leaf of three) per radix level; a 4-wide node takes
    three of them and the rest, so two nodes down the count is 6 at least, where the 63 triangles of a balanced tree need 3."""
    if lds is not None:
        monkeypatch.setenv("RR_STACK_LDS", lds)
    st = B.case(oracle, "chain")
    c = _built(native_lib, st, builder)
    info = c.bvh_info()
    print("chain", builder, lds, info)
    if builder == "gpu":
        assert info["stack_need"] >= 6, info
    if lds is not None:
        assert info["stack_need"] > int(lds), info                            # deeper than the LDS stack in use
    assert_trace_equals_brute_force(c, st, builder, "chain, RR_STACK_LDS=%s" % lds)
    c.close()


# ---- 7. faces without area --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("builder", BUILDERS)
def test_faces_without_area_are_never_hit(native_lib, oracle, builder):
    st = B.case(oracle, "degenerate")
    n = len(st["faces"]) - B.N_DEGENERATE
    c = _built(native_lib, st, builder)
    print("degenerate", builder, c.bvh_info())
    t, face = assert_trace_equals_brute_force(c, st, builder, "with 16 faces without area")
    assert not (face[t >= 0] >= n).any()
    c.close()
    # the scene without them: every hit stays (tests/test_lbvh_host.py says the same of the brute force)
    c = native_lib.Context(0)
    c.set_mesh(st["verts"][:3 * n], st["faces"][:n], None, builder=builder)
    t1, face1 = c.debug_trace(st["o"], st["d"])
    c.close()
    assert np.array_equal(t.view(np.uint32), t1.view(np.uint32)) and np.array_equal(face[t >= 0], face1[t1 >= 0])


# ---- 8. builds do not depend on atomics' arrival order ----------------------------------------------------------------------
def test_three_builds_on_one_context_are_one_tree_to_every_ray(native_lib, oracle):
    st = B.case(oracle, "capped")
    cfg = params.kaist_preset(n_reflections=2, ambient_noise=0)
    pose = scenes.yaw_pose(0.3, -0.4, 0.15, 0.3)                             # 0.15 m above the terrain, between the huge faces
    c = native_lib.Context(0)
    runs = []
    for step in ("set_mesh", "rebuild 1", "rebuild 2"):
        if step == "set_mesh":
            c.set_mesh(st["verts"], st["faces"], None, builder="gpu")
            c.set_materials(params.kaist_materials(), [1], 0)
            c.set_config(cfg, 24)
            c.set_beam_samples(golden_beams(16))
        else:
            c.rebuild_tree("gpu")
        t, face = assert_trace_equals_brute_force(c, st, "gpu", step)
        img, _, stats = c.simulate(pose)
        runs.append((c.bvh_info(), t.copy(), face.copy(), img.copy(), stats))
        print(step, runs[-1][0], "hits", stats["hits"], "bytes set", int((img > 0).sum()))
    c.close()
    assert runs[0][3].any() and runs[0][4]["hits"] > 0
    for info, t, face, img, stats in runs[1:]:
        assert info == runs[0][0], (info, runs[0][0])
        assert np.array_equal(t.view(np.uint32), runs[0][1].view(np.uint32)) and np.array_equal(face, runs[0][2])
        assert img.tobytes() == runs[0][3].tobytes()
        assert stats["hits"] == runs[0][4]["hits"]


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------
def test_gpu_builder_refuses_and_keeps_the_tree(native_lib, oracle):
    """rr_set_mesh_gpu with a face index equal to nv and with a NaN vertex: -4 and a message, the tree stays (the host builder's
    refusals are in test_gpu_parity.py and test_gpu_dynamic.py).  No faces at all is no refusal: the empty mesh is a mesh, every
    ray misses it (test_gpu_parity.py), and rr_set_mesh_gpu hands it to rr_set_mesh.  rr_rebuild_tree takes no geometry: it
    has nothing of this kind to refuse, and rebuilds the tree it is given after each refusal."""
    st = B.case(oracle, "separated:9")
    v, f = st["verts"], st["faces"]
    c = _built(native_lib, st, "gpu")
    info = c.bvh_info()
    before = assert_trace_equals_brute_force(c, st, "gpu", "before")
    bad_f = f.copy(); bad_f[4, 1] = len(v)
    nan_v = v.copy(); nan_v[7, 2] = np.nan
    for verts, faces, text in ((v, bad_f, "face index out of range"), (nan_v, f, "non-finite vertex")):
        with pytest.raises(native_lib.RRError, match=text + r".*\(rc=-4\)"):
            c.set_mesh(verts, faces, None, builder="gpu")
        assert c.bvh_info() == info
        after = assert_trace_equals_brute_force(c, st, "gpu", "after: " + text)
        assert np.array_equal(after[0].view(np.uint32), before[0].view(np.uint32)) and np.array_equal(after[1], before[1])
        c.rebuild_tree("gpu")
        assert c.bvh_info() == info
        assert_trace_equals_brute_force(c, st, "gpu", "rebuilt after: " + text)
    c.set_mesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32), None, builder="gpu")
    t, _ = c.debug_trace(st["o"], st["d"])
    assert (t < 0).all() and c.bvh_info()["n_tris"] == 0
    c.close()
