"""Shared helpers for the parity tests (test infrastructure)."""
import json
import os

import numpy as np
import pytest

from radarays_ros_amd import beams, params, scenes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


from radarays_ros_amd.fixtures import golden_beams, materials_for  # noqa: E402,F401  (shared with bench.py / tools)


def mats_tuple(mats):
    return [m.astuple() for m in mats]


def image_diff(a_f32, b_f32, a_u8, b_u8):
    """SURVEY §8d parity gate: mean(|f32_gpu - f32_cpu|)/255, plus u8 stats."""
    fa = np.nan_to_num(a_f32.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    fb = np.nan_to_num(b_f32.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    d8 = np.abs(a_u8.astype(np.int32) - b_u8.astype(np.int32))
    return {
        "mean_dev": float(np.mean(np.abs(fa - fb)) / 255.0),
        "max_abs_f32": float(np.max(np.abs(fa - fb))),
        "u8_mismatch_frac": float(np.mean(d8 > 0)),
        "u8_gt1_frac": float(np.mean(d8 > 1)),
        "u8_max": int(d8.max()),
    }


def assert_trace_equals_brute_force(c, st, builder, step):
    """t as f32 bits, the face id and the misses, for every ray; the message names the first ray that differs"""
    t, face = c.debug_trace(st["o"], st["d"])
    want_t, want_f = st["t"], st["face"]
    hit = want_t >= 0
    bad = np.where(hit, (t.view(np.uint32) != want_t.view(np.uint32)) | (face != want_f), ~(t < 0))
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        pytest.fail("builder %s, step %s (state %s): %d of %d rays differ; ray %d got (t %r, face %d) wanted (t %r, face %d) "
                    "origin %r direction %r" % (builder, step, st["name"], int(bad.sum()), len(bad), i, float(t[i]), int(face[i]),
                                                 float(want_t[i]), int(want_f[i]), st["o"][i].tolist(), st["d"][i].tolist()))
    return t, face
