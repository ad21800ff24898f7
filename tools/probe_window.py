"""Windowed CFAR on the card, at the north-star target's geometry (BASELINE.md "Windowed CFAR").

    python tools/probe_window.py [--config 4] [--reps 20] [--json out.json]
    python tools/probe_window.py --cases window_os ...      # some cases alone (for rocprofv3 --kernel-trace --stats, or a --pmc run)

Kernel time per 16-frame batch of 400 x 3424 images simulated from the target scene (tools/probe_detect.py's source), from device
events around `--reps` back-to-back calls: rr_detect method 0 (T = 16, G = 2) as the yardstick, then CA, GO, SO and OS of
rr_detect_window_device at the default window (Gr 2, Tr 16, Ga 1, Ta 2), each with its ratio to the yardstick and its points per frame, and OS
again at a rank and scale that find points in these images."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from radarays_ros_amd import native, params, scenes  # noqa: E402
from radarays_ros_amd.fixtures import golden_beams, materials_for  # noqa: E402
from tools.probe_detect import CFAR, F, WORKLOAD, event_ms  # noqa: E402

METHODS = ("ca", "go", "so", "os")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cases", nargs="*", help="cases to time (default: all): cfar_T16_G2, window_ca, window_go, window_so, window_os, window_os_mask, window_os_rank500_scale1.5")
    ap.add_argument("--json")
    a = ap.parse_args()

    t0 = time.time()
    scene = scenes.config_scene(a.config)
    n_pass, n_rays = WORKLOAD[a.config]
    cfg = params.kaist_preset(n_reflections=n_pass, n_samples=n_rays, ambient_noise=2)
    ctx = native.Context(0)
    ctx.set_mesh(scene["verts"], scene["faces"], scene["face_object_id"])
    ctx.set_materials(materials_for(scene), scene["object_materials"], 0)
    ctx.set_config(cfg, params.N_ANGLES)
    ctx.set_beam_samples(golden_beams(n_rays))
    ctx.set_noise_offsets((np.random.RandomState(7).uniform(0, 1, 16 * params.N_ANGLES) * 1000.0).astype(np.float32))
    poses = scenes.trajectory(16, scene["name"])
    print("scene %s, %d triangles, set up in %.1f s" % (scene["name"], len(scene["faces"]), time.time() - t0), flush=True)

    dev = torch.device("cuda", 0)
    A, N = params.N_ANGLES, cfg.n_cells
    s0 = torch.cuda.Stream(device=dev)
    imgs = torch.empty((F, N, A), dtype=torch.uint8, device=dev)
    offs = torch.empty((F, A + 1), dtype=torch.int32, device=dev)
    mask = torch.empty((F, N, A), dtype=torch.uint8, device=dev)
    ctx.simulate_batch_device(poses[:F], imgs.data_ptr(), s0.cuda_stream)
    ctx.synchronize(s0.cuda_stream)
    ptr = imgs.data_ptr()
    out = {"config": a.config, "frames_per_batch": F, "n_cells": N, "n_angles": A, "tile": list(native.detect_window_tile_sizes(None, N, A))}

    def count(det):
        det(None, 0, None)
        ctx.synchronize(s0.cuda_stream)
        return offs[:, -1].cpu().numpy().view(np.uint32)

    def plain(d_pts, mp, d_mask):
        ctx.detect_device(ptr, F, CFAR, d_pts, mp, offs.data_ptr(), s0.cuda_stream)

    def windowed(method, **kw):
        return lambda d_pts, mp, d_mask: ctx.detect_window_device(ptr, F, dict(kw, method=method), d_pts, mp, offs.data_ptr(), d_mask, s0.cuda_stream)

    cases = {"cfar_T16_G2": (plain, False)}
    for m in METHODS:
        cases["window_" + m] = (windowed(m), False)
    cases["window_os_mask"] = (windowed("os"), True)
    cases["window_os_rank500_scale1.5"] = (windowed("os", rank_permille=500, scale=1.5), False)      # an emit pass that has points to write
    if a.cases:
        cases = {k: v for k, v in cases.items() if k in a.cases}
    with torch.cuda.stream(s0):
        for name, (det, with_mask) in cases.items():
            tot = count(det)
            mp = max(1, int(tot.max()))
            pts = torch.empty((F, mp * 24), dtype=torch.uint8, device=dev)
            ms = event_ms(lambda: det(pts.data_ptr(), mp, mask.data_ptr() if with_mask else None), a.reps, s0)
            out[name + "_us_per_batch"] = round(ms * 1000.0, 2)
            out[name + "_points_per_frame"] = float(tot.mean())
            print("%-18s %10.2f us per %d-frame batch, %9.1f points per frame" % (name, ms * 1000.0, F, tot.mean()), flush=True)
    base = out.get("cfar_T16_G2_us_per_batch")
    for name in cases:
        if base and name != "cfar_T16_G2":
            out[name + "_ratio"] = round(out[name + "_us_per_batch"] / base, 2)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
