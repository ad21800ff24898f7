"""orc_column -- the column step of the oracle alone (RadarCPU.cpp:402-542) -- is the loop orc_simulate runs: fed with the
echo stream a sweep logged for an azimuth it gives that azimuth's column of the sweep, bit for bit.  tests/test_oracle_refloop.py,
test_oracle_loop.py and test_oracle_kat.py pin orc_simulate to the reference's compiled loop, and through it orc_column, the
reference tests/test_gpu_column.py holds k_column to.  No GPU."""
import sys

import numpy as np
import pytest

from common import GOLDEN, mats_tuple

sys.path.insert(0, GOLDEN)
import gen_oracle_images as gen  # noqa: E402


def logged_sweep(oracle, case):
    """(cfg, noise offsets or None, (az_begin, az_end), u8, f32, echo log) of one small oracle sweep"""
    s, cfg, mats, beams, pose, az, rnd = case()
    sc = oracle.Scene(s["verts"], s["faces"], s["face_object_id"], use_bvh=0)
    log = {"cap": 2048}
    u8, f32, st = oracle.simulate(sc, mats_tuple(mats), s["object_materials"], cfg, beams, pose, noise_rnd=rnd,
                                  az_begin=az[0], az_end=az[1], echo_log=log)
    assert int(log["counts"].sum()) == st["signals"] and int(log["counts"].max()) <= log["cap"]
    return cfg, rnd, az, u8, f32, log


@pytest.mark.parametrize("case", ["multibounce", "noise"])
def test_orc_column_on_the_logged_stream_is_the_sweeps_column(oracle, case):
    cfg, rnd, az, u8, f32, log = logged_sweep(oracle, gen.CASES[case])
    assert log["counts"][az[0]:az[1]].max() > 0
    for a in range(az[0], az[1]):
        n = int(log["counts"][a])
        col = (cfg.scroll_image + a) % 400
        cf, c8 = oracle.column(cfg, log["cells"][a, :n], log["strengths"][a, :n], 0.0 if rnd is None else rnd[a], col)
        assert np.array_equal(cf.view(np.uint32), f32[:, col].view(np.uint32)), (case, a)
        assert np.array_equal(c8, u8[:, col]), (case, a)


def test_orc_column_drops_what_lies_outside_the_image(oracle):
    """cell < 0 (an empty slot of a stream) and cell >= n_cells are no echoes, with and without the denoiser; bin 0 is never
    written by a window (RadarCPU.cpp:424) but is by the fmaxf path (:439)."""
    from radarays_ros_amd import params
    for den in (0, 1):
        cfg = params.RadarModelConfig()
        cfg.n_cells, cfg.ambient_noise, cfg.signal_denoising = 40, 0, den
        cfg.signal_denoising_triangular_width, cfg.signal_denoising_triangular_mode = 9, 0.35
        keep = (np.array([5, 0, 39], np.int32), np.array([1.0, 2.0, 0.5], np.float32))
        full = (np.array([-1, 5, 40, 0, -3, 45, 39, -2147483648], np.int32), np.array([9, 1.0, 9, 2.0, 9, 9, 0.5, 9], np.float32))
        a, b = oracle.column(cfg, *keep), oracle.column(cfg, *full)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
        assert (a[0][0] == 0.0) == (den == 1) and a[0][5] > 0 and a[0][39] > 0 and np.isfinite(a[0]).all()
