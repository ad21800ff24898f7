"""Dynamic scenes whose faces the tree builders CUT: refit, rebuilt and copied trees against brute force (rr_refit.hip, the
refit state of rr_scene.hip, k_split of rr_lbvh.hip and the spatial splits of rr_bvh.cpp).

The nearest hit does not depend on the tree, so after every step of the refit state machine rr_debug_trace
must give, ray by ray and bit by bit, what the oracle's brute-force loop gives on the posed triangle soup.  The scene
(tests/dynamic_ref.py: split_scene) is one both builders split: a face cut into parts is filed under clipped boxes, and
k_refit_level then keeps the as-built box of a static leaf (widened when the extent has grown), clips a static record in a
mixed leaf, and files a moved record whole.  The rays go where a wrong box shows: at points all over every huge face from
close by, along the planes of the largest faces next to their edges, along the boxes of the static huge faces just outside
them (what only a box widened with the extent catches), and the nasty rays of tests/fuzz/fuzz_trace.py.

There is no tolerance in this file.  The test that is not marked `gpu` builds every state and ray and holds the reference
alone to the conditions that keep the GPU tests from being vacuous."""
import os
import sys

import numpy as np
import pytest

import dynamic_ref as R
from common import assert_trace_equals_brute_force

gpu = pytest.mark.gpu


# ---- the reference alone: every state, its rays, and what keeps the GPU tests from being vacuous ------------------------
def test_every_state_probes_every_huge_face_in_the_reference(oracle):
    s = R.scene()
    nf = len(s["faces"])
    assert 2300 <= nf <= 2700 and len(s["huge"]) == s["n_static_huge"] + 4 and 6 <= s["n_static_huge"] <= 10
    oid = s["face_object_id"]
    assert int(oid.max()) + 1 == R.N_OBJECTS and (oid[s["huge"][:s["n_static_huge"]]] == 0).all() and (oid[s["huge"][-4:]] == 2).all()
    assert 24 <= (oid == 1).sum() // 12 and (oid == 3).sum() == 12 and (oid == 4).sum() == 12
    ext0 = R.extent_measure(R.state(oracle, "built")["soup_verts"])
    for name in R.STATES:
        st = R.state(oracle, name)
        v = st["soup_verts"].reshape(-1, 3, 3).astype(np.float64)
        edge = np.linalg.norm(v[s["huge"]] - np.roll(v[s["huge"]], 1, axis=1), axis=2).max(axis=1)
        assert (edge[:s["n_static_huge"]] >= 20.0).all() and (edge[-4:] >= 15.0).all(), (name, edge)
        assert 6000 <= len(st["o"]) <= 7500
        aimed = st["aim"] >= 0
        assert aimed.sum() == len(s["huge"]) * R.AIMED_PER_FACE
        share = float((st["face"][aimed] == st["aim"][aimed]).mean())
        per_face = np.array([(st["face"] == f).sum() for f in s["huge"]])
        print(name, "aimed rays that hit their face first: %.3f" % share, "nearest hits per huge face:", per_face.tolist(),
              "hits: %d of %d" % ((st["t"] >= 0).sum(), len(st["t"])))
        assert share >= 0.8, (name, share)
        assert (per_face >= 50).all(), (name, per_face)
        # the extent: unchanged where hit_pad must stay, at least threefold where it must grow
        ext = R.extent_measure(st["soup_verts"])
        if R.STATES[name][0] in ("far", "copy"):
            assert ext >= 3.0 * ext0, (name, ext, ext0)
            # ... and there some nearest hits lie on static faces whose boxes, padded as the builders pad them for the extent
            # at the build, the ray never enters: only as-built boxes that were widened let a tree find them (one such ray
            # makes the widening observable; three, so that it does not hang on a single ray)
            hit = st["t"] >= 0
            F = st["face"][hit].astype(np.int64)
            tri = v[F]
            pad = 2e-5 * ext0 + 1e-6
            only_widened = R.misses_boxes(st["o"][hit], st["d"][hit], tri.min(1) - pad, tri.max(1) + pad) & (oid[F] == 0)
            print(name, "nearest hits outside the as-built padding of their static face:", int(only_widened.sum()))
            assert only_widened.sum() >= 3, (name, int(only_widened.sum()))
        else:
            assert ext == ext0, (name, ext, ext0)
    # back at the build poses the soup is the rest mesh, bit for bit
    assert np.array_equal(R.state(oracle, "built")["soup_verts"], s["verts"][s["faces"].reshape(-1)])


# ---- the state machine on one context -----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("builder", ["host", "gpu"])
def test_refit_state_machine_of_a_split_scene_is_bit_exact_vs_brute_force(native_lib, oracle, builder):
    s = R.scene()
    nf = len(s["faces"])
    S = {name: R.state(oracle, name) for name in R.STATES}
    c = native_lib.Context(0)
    c.set_mesh(s["verts"], s["faces"], s["face_object_id"], builder=builder)
    info0 = c.bvh_info()
    print(builder, "records", info0["n_tris"], "faces", nf)
    assert info0["n_tris"] > nf, (builder, info0, nf)                       # the builder did cut faces
    # 0. as built
    t0, f0 = assert_trace_equals_brute_force(c, S["built"], builder, "0 as built")
    # 1. the boxes and the far-off box move inside the extent: static split leaves keep their boxes, mixed leaves clip
    c.set_object_poses(S["inside"]["poses"])
    assert_trace_equals_brute_force(c, S["inside"], builder, "1 moved inside the extent")
    assert c.bvh_info() == info0
    cost1, built = c.tree_cost()
    # 2. the gate turns and shifts: a moved split face, whole under each of its part leaves
    c.set_object_poses(S["gate"]["poses"])
    assert_trace_equals_brute_force(c, S["gate"], builder, "2 gate moved")
    # 3. one box carried far outside: hit_pad grows, the as-built boxes widen
    c.set_object_poses(S["far"]["poses"])
    assert_trace_equals_brute_force(c, S["far"], builder, "3 extent grown")
    assert c.bvh_info() == info0
    # 4. every pose back to what the tree was built with (no update_vertices yet on this context)
    c.set_object_poses(S["built"]["poses"])
    t4, f4 = assert_trace_equals_brute_force(c, S["built"], builder, "4 back at the build poses")
    assert np.array_equal(t4.view(np.uint32), t0.view(np.uint32)) and np.array_equal(f4, f0)
    assert c.tree_cost() == (built, built), (c.tree_cost(), built)
    # 1 again, then its twin: the same rest vertices given anew count as new, every split leaf takes its whole triangle
    c.set_object_poses(S["inside"]["poses"])
    assert c.tree_cost() == (cost1, built)
    c.update_vertices(s["verts"])
    cost1_whole, _ = c.tree_cost()
    print(builder, "tree_cost step 1", cost1, "after update_vertices of the same vertices", cost1_whole, "as built", built)
    assert cost1 < cost1_whole, (cost1, cost1_whole)
    assert_trace_equals_brute_force(c, S["inside"], builder, "1 after update_vertices of the same vertices")
    # 5. a deformed terrain under the poses of step 1: every record counts as moved
    c.update_vertices(S["deformed"]["rest"])
    assert_trace_equals_brute_force(c, S["deformed"], builder, "5 deformed terrain")
    assert c.bvh_info() == info0
    # 6. rebuilds in a posed state, each followed by a pose change: moved[] and the snapshot belong to the rebuilt tree
    c.rebuild_tree("host")
    now, at = c.tree_cost()
    assert abs(now / at - 1.0) < 1e-12
    assert_trace_equals_brute_force(c, S["deformed"], builder, "6 rebuilt (host)")
    c.set_object_poses(S["deformed_gate"]["poses"])
    assert_trace_equals_brute_force(c, S["deformed_gate"], builder, "6 rebuilt (host), gate moved")
    c.rebuild_tree("gpu")
    now, at = c.tree_cost()
    assert abs(now / at - 1.0) < 1e-12
    assert_trace_equals_brute_force(c, S["deformed_gate"], builder, "6 rebuilt (gpu)")
    c.set_object_poses(S["deformed_far"]["poses"])
    assert_trace_equals_brute_force(c, S["deformed_far"], builder, "6 rebuilt (gpu), extent grown")
    c.set_object_poses(S["deformed"]["poses"])
    assert_trace_equals_brute_force(c, S["deformed"], builder, "6 rebuilt (gpu), gate and far box back")
    c.close()


# ---- copies ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("builder", ["host", "gpu"])
def test_copy_of_a_refit_split_tree_is_posed_on_its_own(native_lib, oracle, builder):
    s = R.scene()
    S = {name: R.state(oracle, name) for name in ("inside", "gate", "copy")}
    a = native_lib.Context(0)
    a.set_mesh(s["verts"], s["faces"], s["face_object_id"], builder=builder)
    info0 = a.bvh_info()
    assert info0["n_tris"] > len(s["faces"])
    a.set_object_poses(S["inside"]["poses"])
    a.set_object_poses(S["gate"]["poses"])                                  # the source has been refit twice
    b = native_lib.Context(0)
    b.copy_mesh(a)
    assert b.bvh_info() == info0
    assert_trace_equals_brute_force(b, S["gate"], builder, "7 copy, as copied")
    b.set_object_poses(S["copy"]["poses"])                                  # another way than its source, and the extent grows
    assert_trace_equals_brute_force(b, S["copy"], builder, "7 copy, posed on its own")
    assert_trace_equals_brute_force(a, S["gate"], builder, "7 source, after its copy moved")
    assert a.tree_cost()[1] == b.tree_cost()[1]
    a.close()
    b.set_object_poses(S["inside"]["poses"])                                # the gate is back where the tree was built for it
    assert_trace_equals_brute_force(b, S["inside"], builder, "7 copy, refit after its source closed")
    b.close()


# ---- the split-scene fuzz ---------------------------------------------------------------------------------------------------
@gpu
def test_trace_fuzz_split_scenes_with_grazing_rays(native_lib, oracle):
    """Two scenes of tests/fuzz/fuzz_trace.py's split kind (seeds >= 100000), 2,000 grazing and 1,000 ordinary rays each, both
    builders: the residual class of the grazing guard."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz"))
    import fuzz_trace
    assert fuzz_trace.run(n_seeds=2, first=100000, verbose=False) == 0
