"""The C++ mirror's conversions (RadarHIP::detect / RadarHIP::toCartesian, include/radarays_ros_amd/RadarHIP.hpp), driven
by a plain C++ program, against the numpy restatement (tests/detect_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

import detect_ref as R
from radarays_ros_amd import native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "detect_check.cpp")


def build(tmp_path):
    native.build()
    exe = str(tmp_path / "detect_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), SRC, "-o", exe,
                    "-L", os.path.join(ROOT, "radarays_ros_amd"), "-lradarays_mi355",
                    "-Wl,-rpath," + os.path.join(ROOT, "radarays_ros_amd")], check=True)
    return exe


def test_cpp_mirror_detect_and_cartesian(tmp_path):
    n_cells, n_angles, scroll, k, width, res, ps = 600, 400, 9, 5, 121, 0.0438, 0.25
    rs = np.random.RandomState(4)
    img = rs.randint(0, 30, (n_cells, n_angles)).astype(np.uint8)
    peaks = rs.rand(n_cells, n_angles) < 0.02
    img[peaks] = rs.randint(80, 256, int(peaks.sum()))
    inp = tmp_path / "in.bin"
    with open(inp, "wb") as f:
        f.write(np.array([n_cells, n_angles, scroll, k, width], np.int32).tobytes())
        f.write(np.array([res, ps], np.float32).tobytes())
        f.write(img.tobytes())
    out = tmp_path / "out.bin"
    r = subprocess.run([build(tmp_path), str(inp), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    n_cfar, n_k = np.frombuffer(raw[:16], np.uint64)
    at = 16
    got = []
    for n in (int(n_cfar), int(n_k)):
        got.append(np.frombuffer(raw[at:at + 24 * n], native.POINT_DTYPE))
        at += 24 * n
    cart = np.frombuffer(raw[at:], np.uint8).reshape(width, width)
    g = dict(scroll=scroll, theta_min=0.0, theta_inc=float(np.float32(-2 * np.pi / n_angles)),
             resolution=float(np.float32(res)))
    for pts, det in zip(got, (dict(native.DETECT_DEFAULTS), dict(native.DETECT_DEFAULTS, method=1, k=k))):
        want, _ = R.detect_frame(img, **det, **g)
        assert len(pts) == len(want) > 0
        for key in ("column", "bin", "intensity", "z"):
            assert np.array_equal(pts[key], want[key]), key
        rr = np.hypot(want["x"].astype(np.float64), want["y"].astype(np.float64))
        for key in ("x", "y"):
            assert np.all(np.abs(pts[key].astype(np.float64) - want[key]) <= 1e-6 * rr + 1e-6), key
    d = np.abs(cart.astype(int) - R.cartesian(img, width, ps, True, **g))
    assert d.max() <= 1 and np.mean(d > 0) <= 1e-3
