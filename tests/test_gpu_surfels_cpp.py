"""The C++ RadarHIP::surfacePoints and RadarHIP::registerSurfacePoints (include/radarays_ros_amd/RadarHIP.hpp, through marshal.hpp) on the GPU
against the ctypes path and the numpy restatement (tests/surfels_ref.py), byte for byte: tests/cpp/surfel_check.cpp is compiled with g++
against the library, fed clouds of two walls seen from three poses, and what it writes is compared whole."""
import math
import os
import subprocess

import numpy as np
import pytest

import icp_ref as P
import surfels_ref as R
from radarays_ros_amd import native, params

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ANGLES = 16
CFG = dict(cell=1.0, width=32, min_points=3, max_ratio=0.1)


def walls(rs, step, pose):
    """two perpendicular walls sampled every `step` metres with a little noise, seen from the planar pose (x, y, yaw)"""
    xs, ys = np.arange(-6.0, 6.0, step), np.arange(-4.0, 5.0, step)
    q = np.concatenate([np.stack([xs, np.full_like(xs, 5.0)], -1), np.stack([np.full_like(ys, 6.0), ys], -1)]) + rs.normal(0, 0.01, (len(xs) + len(ys), 2))
    c, s = math.cos(pose[2]), math.sin(pose[2])
    d = q - np.asarray(pose[:2])
    return P.points_of(np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], -1))


@pytest.mark.parametrize("max_surfels, with_init", [(4096, False), (7, True)])
def test_cpp_surfels_equal_the_ctypes_path(tmp_path, max_surfels, with_init):
    native.build()
    exe = str(tmp_path / "surfel_check")
    lib_dir = os.path.join(ROOT, "radarays_ros_amd")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "surfel_check.cpp"), "-o", exe, "-L", lib_dir, "-lradarays_mi355", "-Wl,-rpath," + lib_dir],
                   check=True)
    rs = np.random.RandomState(7)
    clouds = [walls(rs, 0.1, (0, 0, 0)), walls(rs, 0.13, (0.3, -0.2, 0.03)), walls(rs, 0.17, (-0.25, 0.1, -0.02)), np.zeros(0, native.POINT_DTYPE)]
    init = native.se2_states([0.01, -0.01, 0.0], [0.2, -0.2, 0.0], [-0.1, 0.1, 0.0]) if with_init else None
    gate, iterations = 1.0, 6
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.int32([len(clouds), CFG["width"], CFG["min_points"], max_surfels, iterations, int(with_init)]).tobytes())
        f.write(np.float32([CFG["cell"], CFG["max_ratio"], gate]).tobytes() + np.int32([len(c) for c in clouds]).tobytes())
        if with_init:
            f.write(init.tobytes())
        for c in clouds:
            f.write(c.tobytes())
    p = subprocess.run([exe, str(inp), str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    raw = open(out, "rb").read()

    ctx = native.Context(0)
    ctx.set_config(params.kaist_preset(n_cells=64), N_ANGLES)
    offs = np.zeros((len(clouds), N_ANGLES + 1), np.uint32)
    offs[:, -1] = [len(c) for c in clouds]
    surf, counts = ctx.surface_points(clouds, offs, CFG, max_surfels)
    recs = ctx.register_surfels(clouds[1:], offs[1:], surf[0], init, gate, iterations)
    want = counts.tobytes() + b"".join(s.tobytes() for s in surf) + recs.tobytes()
    assert raw == want
    # ... and both are the restatement's bytes
    ref_surf, ref_counts = R.surface_points(clouds, max_surfels=max_surfels, **CFG)
    ref_recs, _, _ = R.register(clouds[1:], ref_surf[0], init, gate, iterations)
    assert want == ref_counts.tobytes() + b"".join(s.tobytes() for s in ref_surf) + ref_recs.tobytes()
    assert counts[0, 0] >= 10 and (counts[0, 1] == R.SF_CAPPED) == (max_surfels == 7) and len(surf[0]) == min(int(counts[0, 0]), max_surfels)
    assert recs["n_matched"][2] == 0 and recs["flags"][2] == R.DEGENERATE                # the empty cloud
    if max_surfels == 4096:                                           # (seven surface points are one wall: a corridor, where the rounding of the pivots decides)
        assert recs["flags"][:2].tolist() == [0, 0] and np.all(recs["n_matched"][:2] > 100)
