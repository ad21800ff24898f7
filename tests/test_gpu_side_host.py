"""The host forms of the frame side chains (rr_simulate_provenance, rr_simulate_paths, rr_simulate_doppler) stage their outputs: a call
that fails AFTER its chain has run -- the frame's error bits come home with the outputs -- has written nothing to any buffer of the
caller's, and the context is as good as new afterwards.  The refusal tests of the three features cover argument errors only, which
fail before anything is launched.  Scene, beams and config are those of tests/test_labels_host.py: with max_waves_per_azimuth = 25
the 24 waves of pass 0 split at the penetrable walls into more than 25, the wave queue overflows (bounds-checked and reported, like
tests/test_gpu_multi.py's cap 61 on 60 beam samples) and every frame fails with code -7."""
import numpy as np
import pytest

import test_labels_host as H
from radarays_ros_amd.native import ECHO_SRC_DTYPE, WAVE_DTYPE, WAVES_MAX_PASSES
from test_gpu_labels import make_ctx, plain

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

A = H.N_ANGLES
SENT = 0x5A
ECHO_STRIDE = 400         # the lane's list holds at most (24 + 48 + 96) * 2 = 336 echoes per azimuth
WAVE_STRIDE = 200         # 24 + 48 + 96 = 168 waves per azimuth at the most
POSE = np.ascontiguousarray(H.POSES[1], np.float32)
V_S = np.float32([1.5, -0.5, 0.25])
CAP = 25


def outputs(n_cells):
    """every output buffer of the three host forms, as bytes filled with the pattern"""
    npx = n_cells * A
    sizes = {"provenance": {"img": npx, "labels": 4 * npx, "faces": 4 * npx, "echoes": A * ECHO_STRIDE * ECHO_SRC_DTYPE.itemsize, "counts": 4 * A},
             "paths": {"img": npx, "waves": A * WAVE_STRIDE * WAVE_DTYPE.itemsize, "counts": 4 * A, "passes": 4 * A * WAVES_MAX_PASSES},
             "doppler": {"img": npx, "f32": 4 * npx, "vel": 4 * A * ECHO_STRIDE, "counts": 4 * A, "cells": 4 * A * ECHO_STRIDE, "vel_img": 4 * npx}}
    return {form: {k: np.full(n, SENT, np.uint8) for k, n in bufs.items()} for form, bufs in sizes.items()}


def call(c, form, b):
    """one host form through the C ABI with every optional output asked for -> its return code"""
    p = {k: v.ctypes.data for k, v in b.items()}
    if form == "provenance":
        return c._L.rr_simulate_provenance(c._h, POSE.ctypes.data, p["img"], p["labels"], p["faces"], p["echoes"], ECHO_STRIDE, p["counts"])
    if form == "paths":
        return c._L.rr_simulate_paths(c._h, POSE.ctypes.data, p["img"], p["waves"], WAVE_STRIDE, p["counts"], p["passes"], 0)
    return c._L.rr_simulate_doppler(c._h, POSE.ctypes.data, V_S.ctypes.data, 0.0, p["img"], p["f32"], p["vel"], ECHO_STRIDE, p["counts"], p["cells"],
                                    p["vel_img"])


def test_a_failure_after_the_chain_writes_nothing_and_leaves_nothing_behind(native_lib):
    cfg = H.config()
    c = make_ctx(native_lib, cfg)
    fresh = make_ctx(native_lib, cfg)
    try:
        # the premise: under this capacity a frame overflows its wave queue, and the library says so
        c.set_config(cfg, A, max_waves_per_azimuth=CAP)
        with pytest.raises(native_lib.RRError, match=r"capacity exceeded.*rc=-7"):
            c.simulate(POSE, 0, A)
        # the failing calls: -7 from each host form, and not a byte of any output has changed
        out = outputs(cfg.n_cells)
        for form, b in out.items():
            assert call(c, form, b) == -7, (form, c._L.rr_last_error(c._h))
            assert b"capacity exceeded" in c._L.rr_last_error(c._h), form
            for k, v in b.items():
                assert (v == SENT).all(), (form, k)
        # recovery on the same context: no sticky error bit, no stale staging
        c.set_config(cfg, A)
        want_img = plain(c, [POSE])[0]
        ref = outputs(cfg.n_cells)
        for form in out:
            assert call(c, form, out[form]) == 0, (form, c._L.rr_last_error(c._h))
            assert call(fresh, form, ref[form]) == 0, (form, fresh._L.rr_last_error(fresh._h))
            # (gain 0: the Doppler image is the plain one too)
            assert np.array_equal(out[form]["img"].reshape(cfg.n_cells, A), want_img), form
            counts = out[form]["counts"].view(np.uint32)
            assert np.array_equal(counts, ref[form]["counts"].view(np.uint32)) and counts.max() > 24, form
            for k in out[form]:          # ... and so is every other byte: rows are written up to their counts, the pattern stays behind them
                assert np.array_equal(out[form][k], ref[form][k]), (form, k)
        assert out["paths"]["counts"].view(np.uint32).max() > CAP          # what the lowered capacity could not hold
        assert np.array_equal(out["provenance"]["counts"], out["doppler"]["counts"])
        c.synchronize()          # nothing is left to report
    finally:
        c.close()
        fresh.close()
