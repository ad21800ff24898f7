"""Point clouds and Cartesian images on the card, at the north-star target's geometry (BASELINE.md "Point clouds").

    python tools/probe_detect.py [--config 4] [--reps 50] [--steps 40] [--json out.json]
    python tools/probe_detect.py --kernels-only [--cases cartesian_1024_nearest ...]   # the conversions alone (for
                                                        # rocprofv3 --kernel-trace --stats, or a --pmc run per case)

1. Kernel time per 16-frame batch of 400 x 3424 images simulated from the target scene, from device events around
   `--reps` back-to-back calls: CA-CFAR (T = 16, G = 2), k-strongest (k = 12), Cartesian 1024 x 1024 bilinear.
2. images/s of simulate-only (rr_simulate_batch_device, images stay in HBM) against simulate + detect (the same, then
   rr_detect_device on the batch's stream, its offsets copied to page-locked host memory, and -- once they have arrived,
   before the slot's buffers are reused -- each frame's true points), with bench.py's three batches in flight (one stream
   and one set of buffers per batch)."""
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

WORKLOAD = {2: (1, 200), 3: (4, 200), 4: (4, 200)}      # config -> (passes, rays per beam), as bench.py's workloads
CFAR = dict(method=0, guard_cells=2, train_cells=16, k=12, min_intensity=1, min_bin=0, cfar_scale=3.0)
KSTRONG = dict(CFAR, method=1)
F = 16                                                   # frames per batch
MAX_POINTS = 400 * 64                                    # per frame: room for what CA-CFAR finds in these images


def event_ms(fn, reps, stream):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=4)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--slots", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--cases", nargs="*", help="kernel cases to time (default: all)")
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
    out = {"config": a.config, "frames_per_batch": F, "n_cells": cfg.n_cells, "n_angles": params.N_ANGLES}
    streams = [torch.cuda.Stream(device=dev) for _ in range(a.slots)]
    imgs = [torch.empty((F, cfg.n_cells, params.N_ANGLES), dtype=torch.uint8, device=dev) for _ in range(a.slots)]
    pts = [torch.empty((F, MAX_POINTS * 24), dtype=torch.uint8, device=dev) for _ in range(a.slots)]
    offs = [torch.empty((F, params.N_ANGLES + 1), dtype=torch.int32, device=dev) for _ in range(a.slots)]
    h_pts = [torch.empty((F, MAX_POINTS * 24), dtype=torch.uint8).pin_memory() for _ in range(a.slots)]
    h_offs = [torch.empty((F, params.N_ANGLES + 1), dtype=torch.int32).pin_memory() for _ in range(a.slots)]
    cart = torch.empty((F, 1024, 1024), dtype=torch.uint8, device=dev)

    s0 = streams[0]
    ctx.simulate_batch_device(poses[:F], imgs[0].data_ptr(), s0.cuda_stream)
    ctx.synchronize(s0.cuda_stream)
    ptr = imgs[0].data_ptr()
    cases = {
        "cfar_T16_G2": lambda: ctx.detect_device(ptr, F, CFAR, pts[0].data_ptr(), MAX_POINTS, offs[0].data_ptr(), s0.cuda_stream),
        "kstrongest_k12": lambda: ctx.detect_device(ptr, F, KSTRONG, pts[0].data_ptr(), MAX_POINTS, offs[0].data_ptr(), s0.cuda_stream),
        "cfar_count_only": lambda: ctx.detect_device(ptr, F, CFAR, None, 0, offs[0].data_ptr(), s0.cuda_stream),
        "cartesian_1024_bilinear": lambda: ctx.polar_to_cartesian_device(ptr, F, 1024, 0.2, cart.data_ptr(), True, s0.cuda_stream),
        "cartesian_1024_nearest": lambda: ctx.polar_to_cartesian_device(ptr, F, 1024, 0.2, cart.data_ptr(), False, s0.cuda_stream),
    }
    if a.cases:
        cases = {k: v for k, v in cases.items() if k in a.cases}
    with torch.cuda.stream(s0):
        for name, fn in cases.items():
            ms = event_ms(fn, a.reps, s0)
            out[name + "_us_per_batch"] = round(ms * 1000.0, 2)
            print("%-26s %8.2f us per %d-frame batch" % (name, ms * 1000.0, F), flush=True)
    for name, det in (("cfar_T16_G2", CFAR), ("kstrongest_k12", KSTRONG)) if not a.cases else ():
        ctx.detect_device(ptr, F, det, None, 0, offs[0].data_ptr(), s0.cuda_stream)
        ctx.synchronize(s0.cuda_stream)
        tot = offs[0][:, -1].cpu().numpy()
        out[name + "_points_per_frame"] = float(tot.mean())
        print("%-26s %8.1f points per frame (max %d)" % (name, tot.mean(), tot.max()), flush=True)
    if a.kernels_only:
        return emit(out, a)

    events = [torch.cuda.Event() for _ in range(a.slots)]
    pending = [False] * a.slots

    def deliver(i):
        """the points of slot i's last batch to the host: its offsets have been copied behind the detection; once they
        are here, each frame's true points follow on the slot's stream (before anything reuses the slot's buffers)"""
        if not pending[i]:
            return
        events[i].synchronize()
        tot = h_offs[i][:, -1].numpy().view(np.uint32)
        assert int(tot.max()) <= MAX_POINTS
        with torch.cuda.stream(streams[i]):
            for f in range(F):
                nb = int(tot[f]) * 24
                if nb:
                    h_pts[i][f, :nb].copy_(pts[i][f, :nb], non_blocking=True)
        pending[i] = False

    def run(detect, steps):
        n = 0
        for k in range(steps):
            for b in range(2):              # two batches of F frames per step
                i = n % a.slots
                s = streams[i]
                ps = [poses[(n * F + f) % len(poses)] for f in range(F)]
                deliver(i)
                ctx.simulate_batch_device(ps, imgs[i].data_ptr(), s.cuda_stream)
                if detect:
                    ctx.detect_device(imgs[i].data_ptr(), F, CFAR, pts[i].data_ptr(), MAX_POINTS, offs[i].data_ptr(), s.cuda_stream)
                    with torch.cuda.stream(s):
                        h_offs[i].copy_(offs[i], non_blocking=True)
                        events[i].record(s)
                    pending[i] = True
                n += 1
        for i in range(a.slots):
            deliver(i)
        torch.cuda.synchronize()
        return n * F

    for detect in (False, True, False, True):        # alternated: the second pair is the one reported
        run(detect, 4)
        t = time.perf_counter()
        frames = run(detect, a.steps)
        ips = frames / (time.perf_counter() - t)
        out["images_per_s_" + ("simulate_detect" if detect else "simulate_only")] = round(ips, 1)
        print("%-26s %10.1f images/s" % ("simulate+detect" if detect else "simulate only", ips), flush=True)
    out["detect_ratio"] = round(out["images_per_s_simulate_detect"] / out["images_per_s_simulate_only"], 4)
    print("ratio %.4f" % out["detect_ratio"])
    return emit(out, a)


def emit(out, a):
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
