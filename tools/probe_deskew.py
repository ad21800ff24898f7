#!/usr/bin/env python
"""Times the sweep compensation calls on one MI355X: a 16-frame batch of 400 x 3424 images through
rr_sweep_table_device, rr_compensate_points_device (on CA-CFAR output), rr_polar_to_cartesian_sweep_device at 1024^2 for nearest /
bilinear and 1, 2, 3 iterations, and, in the same process on the same images, the unchanged rr_polar_to_cartesian_device and
rr_detect_device.  Device events around `reps` back-to-back calls after a warm-up; prints one JSON line.

    python tools/probe_deskew.py [--reps 20] [--only NAME]      (--only: one call in a loop, for a counter run under rocprofv3)
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radarays_ros_amd import native, params, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    n, A, N, W = a.frames, 400, 3424, a.width
    ctx = native.Context(0)
    cfg = params.kaist_preset()
    ctx.set_config(cfg, A)
    res = ctx._rrcfg.resolution
    ps = 2 * N * res / W
    rs = np.random.RandomState(1)
    imgs = rs.randint(0, 30, (n, N, A)).astype(np.uint8)                  # low noise with sparse strong peaks: a radar image's statistics
    peaks = rs.rand(n, N, A) < 0.02
    imgs[peaks] = rs.randint(80, 256, int(peaks.sum()))
    az, ref, vel = [], [], []
    for f in range(n):
        pose = scenes.yaw_pose(1.0 + f, 1.5, 0.2, 0.1 * f)
        p, v = scenes.sweep_poses(pose, [20.0, 0.0, 0.0, 0.0, 0.0, 0.3], 0.25, A, 0)
        az.append(p); ref.append(pose); vel.append(v)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)   # noqa: E731
    d_imgs, d_az, d_ref, d_vel = up(imgs), up(np.stack(az)), up(np.stack(ref).astype(np.float32)), up(np.stack(vel))
    d_tab = torch.zeros(n * A * 32, dtype=torch.uint8, device=dev)
    d_offs = torch.zeros((n, A + 1), dtype=torch.int32, device=dev)
    det = dict(native.DETECT_DEFAULTS)
    ctx.detect_device(d_imgs.data_ptr(), n, det, None, 0, d_offs.data_ptr())
    ctx.synchronize()
    mp = int(d_offs[:, -1].max().item())
    d_pts = torch.zeros(n * mp * 24, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(n * mp * 24, dtype=torch.uint8, device=dev)
    d_cart = torch.zeros((n, W, W), dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    P = lambda t: t.data_ptr()   # noqa: E731
    calls = {
        "sweep_table": lambda: ctx.sweep_table_device(P(d_az), P(d_ref), n, P(d_tab), P(d_vel), 0.05, s),
        "detect_cfar": lambda: ctx.detect_device(P(d_imgs), n, det, P(d_pts), mp, P(d_offs), s),
        "compensate_points": lambda: ctx.compensate_points_device(P(d_pts), P(d_offs), n, mp, P(d_tab), P(d_out), s),
    }
    for bil in (False, True):
        name = "bilinear" if bil else "nearest"
        calls["cartesian_plain_" + name] = (lambda bil=bil: ctx.polar_to_cartesian_device(P(d_imgs), n, W, ps, P(d_cart), bil, s))
        for it in (1, 2, 3):
            calls["cartesian_sweep_%s_it%d" % (name, it)] = (
                lambda bil=bil, it=it: ctx.polar_to_cartesian_sweep_device(P(d_imgs), n, W, ps, P(d_tab), P(d_cart), bil, it, s))
    calls["sweep_table"](); calls["detect_cfar"]()
    ctx.synchronize(s)
    names = [a.only] if a.only else list(calls)
    out = {"frames": n, "n_cells": N, "n_angles": A, "width": W, "reps": a.reps, "points_per_frame": mp, "us_per_batch": {}}
    with torch.cuda.stream(stream):
        for name in names:
            fn = calls[name]
            for _ in range(3):
                fn()
            ctx.synchronize(s)
            rounds = []
            for _ in range(3):                                            # three rounds of `reps` calls: the median round is reported
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for _ in range(a.reps):
                    fn()
                e1.record(stream)
                e1.synchronize()
                rounds.append(e0.elapsed_time(e1) * 1e3 / a.reps)
            out["us_per_batch"][name] = {"median": round(sorted(rounds)[1], 2), "min": round(min(rounds), 2), "max": round(max(rounds), 2)}
    u = out["us_per_batch"]
    if not a.only:
        out["ratio_sweep_over_plain"] = {k: round(u[k]["median"] / u["cartesian_plain_" + k.split("_")[2]]["median"], 3) for k in u if k.startswith("cartesian_sweep")}
        out["share_of_detect"] = {k: round(u[k]["median"] / u["detect_cfar"]["median"], 4) for k in ("sweep_table", "compensate_points")}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
