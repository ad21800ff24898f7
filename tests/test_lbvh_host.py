"""The CPU side of the tree-builder edge tests (tests/test_gpu_lbvh_edges.py): the reference of every case held to what keeps
the GPU tests from being vacuous, and the covering property the trace tests rely on, on k_split / clip_tri_box of rr_lbvh.hip
restated in numpy f32 (tests/lbvh_ref.py).  No GPU."""
import numpy as np
import pytest

import dynamic_ref as R
import lbvh_ref as B


@pytest.mark.parametrize("name", B.CASES)
def test_reference_of_every_case(oracle, name):
    st = B.case(oracle, name)
    v, f = st["verts"], st["faces"]
    assert len(f) <= 3000 and 2000 <= len(st["o"]) <= 4000, (len(f), len(st["o"]))
    hit = st["t"] >= 0
    assert 0.3 * len(hit) < hit.sum() < len(hit)                             # hits and misses
    # no ray of the grazing guard's residual class: every ray is compared, none needs an excuse
    assert B.residual_class(v, f, st["o"], st["d"], st["t"], st["face"]).sum() == 0
    aimed = st["aim"] >= 0
    share = float((st["face"][aimed] == st["aim"][aimed]).mean())
    print(name, "faces", len(f), "rays", len(hit), "hits", int(hit.sum()), "aimed rays that hit their face first: %.3f" % share)
    kind = name.split(":")[0]
    if kind == "separated":
        assert len(f) == int(name.split(":")[1]) and share == 1.0
        tri = v[f]
        side = (tri.max(1) - tri.min(1)).max(1)
        assert side.max() < 0.9 and np.unique(st["face"][hit]).size == len(f)    # every triangle is somebody's nearest hit
    if kind == "capped":
        for h in st["huge"]:
            mine = st["aim"] == h
            assert mine.sum() >= 50
            assert (st["face"][mine] == h).mean() >= 0.8, (name, h)
            assert (st["face"] == h).sum() >= 50
    if kind == "chain":
        assert np.unique(st["face"][hit]).size == len(f) == 63
    if kind in ("flat", "strip"):
        ext = v.max(0) - v.min(0)
        assert (ext[2] == 0.0) if kind == "flat" else (ext[0] == 400.0 and ext[1] == 0.5 and ext[2] == 0.5)
    if kind == "degenerate":
        n = len(f) - B.N_DEGENERATE
        assert not (st["face"][hit] >= n).any()                              # no hit on a face without area ...
        t, face = R.brute_force(oracle, v, f[:n], st["o"], st["d"])          # ... and none lost or won to one
        assert np.array_equal(t.view(np.uint32), st["t"].view(np.uint32)) and np.array_equal(face, st["face"])
        tri = v[f[n:]].astype(np.float64)
        assert (np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1) == 0.0).all()
        assert np.array_equal(tri.astype(np.float32), tri)
        assert ((tri.max(1) - tri.min(1)).min(1) > 5.0).sum() >= 2               # boxes that span cells in every axis


def test_far_case_is_the_near_one_translated_and_recomputed(oracle):
    a, b = B.case(oracle, "capped"), B.case(oracle, "capped:far")
    assert np.abs(b["verts"].astype(np.float64) - a["verts"] - B.FAR_OFFSET).max() < 5e-4      # half an ulp at 6000 m
    assert not np.array_equal(b["t"], a["t"]) and (b["face"] == a["face"]).mean() > 0.95         # its own brute force


def test_coincident_boxes_give_equal_morton_codes_in_bulk():
    v, f, _ = B.scene("coincident")
    tri = v[f]
    key = B.morton_keys(v, tri.min(1), tri.max(1))
    _, count = np.unique(key, return_counts=True)
    assert count.max() >= 300 and (count == 2).sum() >= 140, np.sort(count)[-4:]      # more equal keys than a launch block holds
    side = (tri.max(1) - tri.min(1)).max(1)
    assert side[:300].min() < 0.3 and side[:300].max() > 5.0


def test_huge_faces_reach_the_cell_cap_at_every_lattice_cell():
    for name in ("capped", "capped:far"):
        v, f, huge = B.scene(name)
        tri = v[f[huge]]
        longest = (tri.max(1) - tri.min(1)).max(1)
        # the restated bisection (B.settle_cell, too slow for a test) settles on L = 0.0445 m (0.0449 m far off): 2,469 and
        # 2,468 references, every cut one a part of the two huge faces
        assert (longest > B.K_MAX_CELLS * 0.05).all()
        tri_all = v[f]
        cut = (tri_all.max(1) - tri_all.min(1)).max(1) > B.cut_threshold(v, f)
        assert np.array_equal(np.flatnonzero(cut), huge)                      # the terrain is below the builder's size gate
        capped = [int((longest > B.K_MAX_CELLS * L).sum()) for L in B.lattice_cells(v)]
        assert capped[-1] == 2 and capped[0] == 0, capped                     # the lattice runs across the cap


@pytest.mark.parametrize("name", ["capped", "capped:far"])
def test_parts_of_a_huge_face_cover_it(name):
    """the union of the boxes k_split files a face under contains the face: 2,000 points per face and cell size"""
    v, f, huge = B.scene(name)
    org = v.min(0)
    for L in B.lattice_cells(v):
        for h in huge:
            a, b, c = v[f[h]]
            lo, hi, cell = B.split_face(a, b, c, L, org)
            assert len(lo) > 1
            p = B.sample_face(np.random.RandomState(int(h)), v[f[h]], 2000)
            inside = ((p[:, None, :] >= lo[None]) & (p[:, None, :] <= hi[None])).all(2)
            lost = ~inside.any(1)
            if lost.any():
                i = int(np.flatnonzero(lost)[0])
                gap = np.maximum(np.maximum(lo - p[i], p[i] - hi), 0.0).max(1)
                k = int(np.argmin(gap))
                pytest.fail("%s, L %r, face %d: %d of 2000 points in no part; point %r is %.3g m outside the nearest part, cell %r "
                            "box %r .. %r" % (name, L, h, int(lost.sum()), p[i].tolist(), gap[k], cell[k].tolist(), lo[k].tolist(), hi[k].tolist()))


@pytest.mark.parametrize("n", B.COUNTS)
def test_congruent_triangles_are_below_the_size_gate(n):
    """the restated k_side: no face of the separated scenes is more than twice the mean long, so none is cut"""
    v, f, _ = B.scene("separated:%d" % n)
    tri = v[f]
    assert ((tri.max(1) - tri.min(1)).max(1) <= B.cut_threshold(v, f)).all()
    lo, hi, face = B.split_mesh(v, f, f32_cell := np.float32(0.05))
    assert len(face) == n and np.array_equal(lo, tri.min(1)) and np.array_equal(hi, tri.max(1)), f32_cell
