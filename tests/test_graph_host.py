"""Pose-graph optimisation without a GPU: the symbols and the layouts of its three records, the restatement (tests/graph_ref.py) against
an independent finite difference of the stated cost and against an independent dense Gauss-Newton written here with trigonometry and
np.linalg.solve, and the refusals of the size functions."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import graph_ref as R
from radarays_ros_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "radarays_mi355.h")


def test_symbols_and_layouts(native_lib, tmp_path):
    L = native_lib.lib()
    for name in ("rr_graph_tile_sizes", "rr_graph_plan_bytes", "rr_graph_scratch_bytes", "rr_graph_plan", "rr_graph_plan_device", "rr_optimize_graph",
                 "rr_optimize_graph_device"):
        assert hasattr(L, name) and name in native_lib.PROTOTYPES
    assert L.rr_abi_version() == 7 and "#define RR_ABI_VERSION 7" in open(HEADER).read()
    fields = {"rr_graph_edge": ["i", "j", "c", "s", "tx", "ty", "w_t", "w_r"], "rr_graph_config": ["iterations", "cg_iterations", "lambda", "robust_k", "reserved_"],
              "rr_graph_rec": ["chi2", "n_used", "n_flipped", "n_bad", "n_dead", "cg_stop", "reserved_"]}
    lines = []
    for s, fs in fields.items():
        lines.append('printf("%%zu", sizeof(%s));' % s)
        lines += ['printf(" %%zu", offsetof(%s, %s));' % (s, f) for f in fs]
        lines.append('printf("\\n");')
    (tmp_path / "l.c").write_text('#include <stdio.h>\n#include <stddef.h>\n#include "radarays_mi355.h"\nint main(){%s return 0;}\n' % "\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "l.c"), "-o", str(tmp_path / "l")], check=True)
    rows = [[int(v) for v in r.split()] for r in subprocess.run([str(tmp_path / "l")], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert rows == [[48, 0, 4, 8, 16, 24, 32, 40, 44], [32, 0, 4, 8, 16, 24], [32, 0, 8, 12, 16, 20, 24, 28]]
    for (s, fs), row in zip(fields.items(), rows):
        cls, dt = native.STRUCTS[s]
        assert C.sizeof(cls) == row[0] and [getattr(cls, f).offset for f in fs] == row[1:]
        if dt is not None:
            assert dt.itemsize == row[0] and [dt.fields[f][1] for f in fs] == row[1:]
    assert native.GRAPH_EDGE_DTYPE == R.EDGE_DTYPE and native.GRAPH_REC_DTYPE == R.REC_DTYPE
    text = open(HEADER).read()
    assert re.search(r"RR_GRAPH_EDGE_FLIPPED 1u", text) and re.search(r"RR_GRAPH_EDGE_BAD\s+2u", text) and "Full 3 x 3 information" not in text
    assert "full 3 x 3 information matrices" in text                  # out of scope, and said so


# ---- an independent statement of the cost: angles, atan2 and tan -------------------------------------------------------------------
def angle_cost(x, edges):
    """chi2 from (yaw, tx, ty) per node with the half-angle tangent taken by math.tan"""
    total = 0.0
    for e in edges:
        yi, xi, yi_ = x[e["i"]]
        yj, xj, yj_ = x[e["j"]]
        dx, dy = xj - xi, yj_ - yi_
        ex = math.cos(yi) * dx + math.sin(yi) * dy - e["tx"]
        ey = -math.sin(yi) * dx + math.cos(yi) * dy - e["ty"]
        phi = (yj - yi) - math.atan2(e["s"], e["c"])
        er = 2.0 * math.tan(phi / 2.0)
        total += float(e["w_t"]) * (ex * ex + ey * ey) + float(e["w_r"]) * er * er
    return total


def five_nodes():
    rs = np.random.RandomState(3)
    yaw, tx, ty = rs.uniform(-1, 1, 5), rs.uniform(-3, 3, 5), rs.uniform(-3, 3, 5)
    i, j = np.array([0, 1, 2, 3, 4, 0, 3]), np.array([1, 2, 3, 4, 0, 2, 1])
    truth = R.states_of(yaw, tx, ty)
    z = R.noisy(rs, R.relative(truth[i], truth[j]), 0.2, 0.3)
    return yaw, tx, ty, R.edges_of(i, j, z, rs.uniform(1, 5, 7), rs.uniform(1, 5, 7))


def test_the_gradient_is_the_finite_difference_of_the_stated_cost():
    """2 * J^T W e of the restatement against a central difference of angle_cost.  The update turns a node by 2 atan(dth / 2), moves it by
    (dx, dy).  The tolerance per component is derived, not observed: a central difference at step h is off by C h^2 + O(h^4), so
    D(h) - D(h/2) = (3/4) C h^2 and D(h/2) is off by |D(h) - D(h/2)| / 3 (doubled here for the h^4 term), plus the rounding of the two
    costs, 2 * 2^-52 * chi2 * (number of additions, below 64) / (h/2)."""
    yaw, tx, ty, edges = five_nodes()
    x0 = np.stack([yaw, tx, ty], axis=1)
    g = 2.0 * R.gradient(R.states_of(yaw, tx, ty), np.zeros(5), edges)
    chi2 = angle_cost(x0, edges)
    assert abs(chi2 - R.cost(R.states_of(yaw, tx, ty), edges)) < 1e-12 * chi2

    def diff(n, comp, h):
        out = []
        for sign in (1.0, -1.0):
            x = x0.copy()
            x[n, comp] += 2.0 * math.atan(sign * h / 2.0) if comp == 0 else sign * h
            out.append(angle_cost(x, edges))
        return (out[0] - out[1]) / (2.0 * h)

    h = 1e-3
    worst = 0.0
    for n in range(5):
        for comp in range(3):
            d1, d2 = diff(n, comp, h), diff(n, comp, h / 2)
            tol = 2.0 * abs(d1 - d2) / 3.0 + 2.0 * 2.0 ** -52 * chi2 * 64 / (h / 2)
            worst = max(worst, abs(d2 - g[n, comp]) / tol)
            assert abs(d2 - g[n, comp]) <= tol, (n, comp, d2, g[n, comp], tol)
    assert np.abs(g).max() > 1.0
    print("gradient: worst error / tolerance %.3f" % worst)


# ---- an independent dense Gauss-Newton -------------------------------------------------------------------------------------------------
def dense_gauss_newton(x, fixed, edges, iterations):
    """(yaw, tx, ty) per node; the Jacobian by its trigonometric form, H assembled densely over the free nodes, np.linalg.solve"""
    x = x.copy()
    free = [n for n in range(len(x)) if not fixed[n]]
    col = {n: 3 * k for k, n in enumerate(free)}
    for _ in range(iterations):
        J, W, r = np.zeros((3 * len(edges), 3 * len(free))), np.zeros(3 * len(edges)), np.zeros(3 * len(edges))
        for k, e in enumerate(edges):
            i, j = int(e["i"]), int(e["j"])
            c, s = math.cos(x[i, 0]), math.sin(x[i, 0])
            dx, dy = x[j, 1] - x[i, 1], x[j, 2] - x[i, 2]
            ux, uy = c * dx + s * dy, -s * dx + c * dy
            half = ((x[j, 0] - x[i, 0]) - math.atan2(e["s"], e["c"])) / 2.0
            r[3 * k:3 * k + 3] = [ux - e["tx"], uy - e["ty"], 2.0 * math.tan(half)]
            W[3 * k:3 * k + 3] = [e["w_t"], e["w_t"], e["w_r"]]
            sec2 = 1.0 / math.cos(half) ** 2
            if i in col:
                J[3 * k:3 * k + 3, col[i]:col[i] + 3] = [[uy, -c, -s], [-ux, s, -c], [-sec2, 0, 0]]
            if j in col:
                J[3 * k:3 * k + 3, col[j]:col[j] + 3] = [[0, c, s], [0, -s, c], [sec2, 0, 0]]
        d = np.linalg.solve(J.T @ (W[:, None] * J), -(J.T @ (W * r)))
        for n in free:
            x[n, 0] += 2.0 * math.atan(d[col[n]] / 2.0)
            x[n, 1:] += d[col[n] + 1:col[n] + 3]
    return x


@pytest.mark.parametrize("n_nodes, n_edges, seed", [(3, 3, 1), (12, 20, 2)])
def test_the_restatement_converges_where_a_dense_gauss_newton_does(n_nodes, n_edges, seed):
    """Both run to convergence from one start.  They differ in summation order and in the linear solver only (CG to its floor against an LU),
    so they meet to rounding: measured here 8.9e-16 (3 nodes) and 5.3e-15 (12 nodes) in the largest coordinate difference, on coordinates of
    up to 20 m whose last bit is 3.6e-15.  The bound is 1e-12: about two hundred times the measured."""
    start, fixed, edges = R.random_graph(seed, n_nodes, n_edges)
    got, recs, _ = R.optimize(start, fixed, edges, iterations=25, cg_iterations=3 * n_nodes + 10)
    x0 = np.stack([np.arctan2(start[:, 1], start[:, 0]), start[:, 2], start[:, 3]], axis=1)
    want = dense_gauss_newton(x0, fixed, edges, 25)
    dev = max(np.abs(got[:, 2:] - want[:, 1:]).max(), np.abs(np.angle(np.exp(1j * (np.arctan2(got[:, 1], got[:, 0]) - want[:, 0])))).max())
    print("dense Gauss-Newton, %d nodes: deviation %.3g, chi2 %.6g" % (n_nodes, dev, recs["chi2"][-1]))
    assert dev < 1e-12 and recs["chi2"][-1] < recs["chi2"][0]
    assert np.abs(np.hypot(got[:, 0], got[:, 1]) - 1.0).max() < 1e-15


def test_size_functions_refuse_bad_shapes(native_lib):
    L = native_lib.lib()
    g = native.graph_config(3, 10)
    assert L.rr_graph_plan_bytes(1, 0) > 0 and L.rr_graph_scratch_bytes(1, 0, C.byref(g)) > 0
    assert L.rr_graph_plan_bytes(1 << 20, 1 << 22) > 0 and L.rr_graph_scratch_bytes(1 << 20, 1 << 22, C.byref(g)) > (1 << 22) * 97
    for n, e in ((0, 1), (-1, 1), ((1 << 20) + 1, 1), (1, -1), (1, (1 << 22) + 1)):
        assert L.rr_graph_plan_bytes(n, e) == 0 and L.rr_graph_scratch_bytes(n, e, C.byref(g)) == 0
    assert L.rr_graph_scratch_bytes(4, 4, None) == 0
    for field, v in (("iterations", 257), ("iterations", -1), ("cg_iterations", 1025), ("cg_iterations", -1), ("lambda", -1.0), ("lambda", float("nan")),
                     ("robust_k", -1.0), ("robust_k", float("inf"))):
        bad = native.graph_config(3, 10)
        setattr(bad, field, v)
        assert L.rr_graph_scratch_bytes(4, 4, C.byref(bad)) == 0, field
    bad = native.graph_config(3, 10)
    bad.reserved_[0] = 1
    assert L.rr_graph_scratch_bytes(4, 4, C.byref(bad)) == 0
    # the plan grows with both counts, the scratch with the CG steps too (a word and a scalar per step)
    assert L.rr_graph_plan_bytes(100, 50) < L.rr_graph_plan_bytes(101, 50) <= L.rr_graph_plan_bytes(104, 54)
    assert L.rr_graph_scratch_bytes(4, 4, C.byref(native.graph_config(3, 10))) < L.rr_graph_scratch_bytes(4, 4, C.byref(native.graph_config(3, 1000)))
    # a null context is refused before anything else, without a GPU
    assert L.rr_graph_plan(None, None, 4, 0, None, 0) == -1 and L.rr_optimize_graph(None, None, None, None, 4, 0, None, None, None, None) == -1
    a, b = native.graph_tile_sizes()
    assert (a, b) == (R.CHUNK, R.CHUNK)
    for bad in (dict(n_nodes=0, n_edges=0), dict(n_nodes=1, n_edges=-1)):
        with pytest.raises(ValueError):
            native.Context.graph_plan_bytes(**bad)


def test_graph_edges_packs_matcher_records():
    recs = np.zeros(3, native.ICP_DTYPE)
    recs["c"], recs["s"], recs["tx"], recs["ty"] = [1.0, 0.0, 0.6], [0.0, 1.0, 0.8], [1, 2, 3], [4, 5, 6]
    e = native.graph_edges([0, 1, 2], [1, 2, 0], recs, 4.0, [1.0, 2.0, 3.0])
    assert e.dtype == native.GRAPH_EDGE_DTYPE and e["i"].tolist() == [0, 1, 2] and e["j"].tolist() == [1, 2, 0]
    assert e["c"].tolist() == [1.0, 0.0, 0.6] and e["ty"].tolist() == [4, 5, 6] and e["w_t"].tolist() == [4.0] * 3 and e["w_r"].tolist() == [1.0, 2.0, 3.0]
    assert native.graph_edges([0], [1], native.se2_states(0.0, 1.0, 2.0)).tobytes() == R.edges_of([0], [1], [[1.0, 0.0, 1.0, 2.0]]).tobytes()
    for bad in (dict(i=[0, 1], j=[1], states=recs[:2]), dict(i=[0.5], j=[1], states=recs[:1]), dict(i=[0], j=[1], states=recs), dict(i=[-1], j=[1], states=recs[:1])):
        with pytest.raises(ValueError):
            native.graph_edges(**bad)
