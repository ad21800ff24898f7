"""The C++ RadarHIP::optimizePoseGraph (include/radarays_ros_amd/RadarHIP.hpp, through marshal.hpp) on the GPU against the ctypes path and the
numpy restatement (tests/graph_ref.py), byte for byte: tests/cpp/graph_check.cpp is compiled with g++ against the library, fed a drifting
loop with closures, and what it writes is compared whole."""
import os
import subprocess

import pytest

import graph_ref as R
from radarays_ros_amd import native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("robust_k, lam", [(0.0, 0.0), (1.0, 1e-3)])
def test_cpp_pose_graph_equals_the_ctypes_path(tmp_path, robust_k, lam):
    native.build()
    exe = str(tmp_path / "graph_check")
    lib_dir = os.path.join(ROOT, "radarays_ros_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "graph_check.cpp"), "-o", exe, "-L", lib_dir, "-lradarays_mi355", "-Wl,-rpath," + lib_dir],
                   check=True)
    _, start, fixed, edges = R.loop_graph(12, per_side=6, closures=((0, -1), (3, 15)), outliers=((4, 17, 2.0, 1.0),))
    cfg = dict(iterations=4, cg_iterations=20, lam=lam, robust_k=robust_k)
    g = native.graph_config(**cfg)
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np_i32([len(start), len(edges)]) + bytes(g) + start.tobytes() + fixed.tobytes() + edges.tobytes())
    p = subprocess.run([exe, str(inp), str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    raw = open(out, "rb").read()
    states, recs = native.Context(0).optimize_graph(start, fixed, edges, cfg)
    assert raw == states.tobytes() + recs.tobytes()
    want = R.optimize(start, fixed, edges, **cfg)                      # ... and both are the restatement's bytes
    assert raw == want[0].tobytes() + want[1].tobytes()
    assert states.tobytes() != start.tobytes() and recs["chi2"][-1] < recs["chi2"][0]


def np_i32(v):
    import numpy as np
    return np.int32(v).tobytes()
