"""The C++ mirror's windowed CFAR (RadarHIP::detectWindow over marshal::detect_window, include/radarays_ros_amd/), driven by a plain C++
program (tests/cpp/window_check.cpp): it builds with the warnings on and refuses a short input without a device, and on the GPU its
points and masks equal the ctypes path's byte for byte."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from radarays_ros_amd import native, params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "window_check.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    native.build()
    out = str(tmp_path_factory.mktemp("window_check") / "window_check")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-o", out,
                        "-L", os.path.join(ROOT, "radarays_ros_amd"), "-lradarays_mi355", "-Wl,-rpath," + os.path.join(ROOT, "radarays_ros_amd")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_driver_builds_and_refuses_a_short_input(exe, tmp_path):
    """(the input is read before a context is made, so this needs no device)"""
    short = tmp_path / "short.bin"
    short.write_bytes(np.array([64, 16, 0, 1], np.int32).tobytes())
    r = subprocess.run([exe, str(short), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "short" in r.stderr
    assert not (tmp_path / "out.bin").exists()
    assert subprocess.run([exe], capture_output=True, text=True, timeout=120).returncode == 2


CONFIGS = [dict(), dict(method="ca", scale=2.0), dict(method="go"), dict(method="so", min_bin=7, min_intensity=20),
           dict(method="os", guard_range=0, train_range=1, guard_azimuth=0, train_azimuth=1, rank_permille=500, scale=1.5),
           dict(method="os", scale=250.0)]                                       # the last one finds nothing


@pytest.mark.gpu
def test_cpp_detect_window_equals_the_ctypes_path_byte_for_byte(exe, tmp_path):
    n_cells, n_angles, scroll, res = 300, 400, 9, 0.0438
    rs = np.random.RandomState(4)
    img = rs.randint(0, 30, (n_cells, n_angles)).astype(np.uint8)
    peaks = rs.rand(n_cells, n_angles) < 0.02
    img[peaks] = rs.randint(80, 256, int(peaks.sum()))
    img[140:150, :] = 200
    cfgs = [native.window_detect_config(c, n_cells=n_cells, n_angles=n_angles) for c in CONFIGS]
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        f.write(np.array([n_cells, n_angles, scroll, len(cfgs)], np.int32).tobytes())
        f.write(np.array([res], np.float32).tobytes())
        for c in cfgs:
            f.write(bytes(c))
        f.write(img.tobytes())
    r = subprocess.run([exe, str(inp), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    raw = open(out, "rb").read()
    ctx = native.Context(0)
    ctx.set_config(params.kaist_preset(n_cells=n_cells, scroll_image=scroll, resolution=float(np.float32(res))), n_angles)
    at, found = 0, 0
    for c in cfgs:
        n = int(np.frombuffer(raw[at:at + 8], np.uint64)[0])
        at += 8
        pts, _, mask = ctx.detect_window(img, c, mask=True)
        assert n == len(pts[0])
        assert raw[at:at + 24 * n] == pts[0].tobytes()
        at += 24 * n
        assert raw[at:at + img.size] == mask[0].tobytes()
        at += img.size
        found += n
    assert at == len(raw) and found > 0
    assert C.sizeof(native.RRWindowDetectConfig) == 48
