#!/usr/bin/env python
"""Times the oriented surface points and the point-to-line scan matcher on one MI355X, on the clouds of
tools/probe_icp.py: 64 clouds of about 4,800 points, a target of 4,800 points.  rr_surface_points_device on the 64 clouds (8 m cells, 32 x
32 of them, every sample kept); rr_register_surfels_device of the 64 clouds against the target's surface points at 10 iterations.  Device
events around `reps` back-to-back calls after a warm-up; the time per (pass, solve) pair is the call at 10 iterations minus the call at 0
iterations, over 10, as probe_icp.py takes it.  Beside it the model: distance evaluations * 8 VALU operations at the chip's fp32 vector
issue rate.  Prints one JSON line.

    python tools/probe_surfels.py [--reps 10]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radarays_ros_amd import native, params  # noqa: E402

LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9      # tools/probe_icp.py says where this comes from
OPS_PER_EVAL = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--points", type=int, default=4800)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--frames", type=int, default=64)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    A, P, IT, n = 400, a.points, a.iterations, a.frames
    ctx = native.Context(0)
    ctx.set_config(params.kaist_preset(), A)
    rs = np.random.RandomState(1)
    tgt_xy = rs.uniform(-100, 100, (P, 2))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)   # noqa: E731

    def cloud(xy):
        p = np.zeros(len(xy), native.POINT_DTYPE)
        p["x"], p["y"] = xy[:, 0], xy[:, 1]
        return p

    pts = np.zeros((n, P), native.POINT_DTYPE)
    offs = np.zeros((n, A + 1), np.uint32)
    for f in range(n):
        m = P - rs.randint(0, 64)
        yaw, t = rs.uniform(-0.035, 0.035), rs.uniform(-0.5, 0.5, 2)
        q = tgt_xy[rs.permutation(P)[:m]] + rs.normal(0, 0.05, (m, 2)) - t
        c, sn = math.cos(yaw), math.sin(yaw)
        pts[f, :m] = cloud(np.stack([c * q[:, 0] + sn * q[:, 1], -sn * q[:, 0] + c * q[:, 1]], -1))
        offs[f, -1] = m
    cfg = native.surfel_config(8.0, 32, 3, 1.0)
    cap = 1024
    t_offs = np.zeros((1, A + 1), np.uint32)
    t_offs[0, -1] = P
    surf, counts = ctx.surface_points([cloud(tgt_xy)], t_offs, cfg, cap)
    T = len(surf[0])
    d_pts, d_offs, d_tgt, d_cnt = up(pts), up(offs), up(surf[0]), up(np.array([T], np.uint32))
    d_rec = torch.zeros(n * native.ICP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_surf = torch.zeros(n * cap * native.SURFEL_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_counts = torch.zeros(n * 8, dtype=torch.uint8, device=dev)
    need = ctx.surfels_scratch_bytes(n, cfg)
    d_scratch = torch.zeros(need, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    P_ = lambda t: t.data_ptr()   # noqa: E731

    def timed(fn):
        for _ in range(2):
            fn()
        ctx.synchronize(s)
        rounds = []
        for _ in range(3):                                                # three rounds of `reps` calls: the median round is reported
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.reps):
                fn()
            e1.record(stream)
            e1.synchronize()
            rounds.append(e0.elapsed_time(e1) * 1e3 / a.reps)
        return {"median": round(sorted(rounds)[1], 1), "min": round(min(rounds), 1), "max": round(max(rounds), 1)}

    out = {"frames": n, "points": P, "target_points": P, "target_surfels": T, "iterations": IT, "reps": a.reps, "scratch_bytes": need,
           "tiles": native.surfels_tile_sizes()}
    with torch.cuda.stream(stream):
        out["surface_points_us_per_call"] = timed(lambda: ctx.surface_points_device(P_(d_pts), P_(d_offs), n, P, cfg, P_(d_surf), cap, P_(d_counts),
                                                                                    P_(d_scratch), need, s))
        us = {it: timed(lambda it=it: ctx.register_surfels_device(P_(d_pts), P_(d_offs), n, P, P_(d_tgt), P_(d_cnt), T, P_(d_rec), None, 2.0, it, None, s))
              for it in (0, IT)}
    kept = d_counts.cpu().numpy().view(np.uint32).reshape(n, 2)
    rec = d_rec.cpu().numpy().view(native.ICP_DTYPE)
    evals = float(offs[:, -1].sum()) * T
    per_pass = (us[IT]["median"] - us[0]["median"]) / IT
    model_pass = evals * OPS_PER_EVAL / LANE_OPS_PER_S * 1e6
    out.update({"mean_kept": float(kept[:, 0].mean()), "register_us_per_call_0_iterations": us[0], "register_us_per_call": us[IT],
                "us_per_pass_solve_pair": round(per_pass, 1), "evaluations_per_pass": evals, "model_us_per_pass": round(model_pass, 2),
                "measured_over_model": round(per_pass / model_pass, 2), "mean_matched": float(rec["n_matched"].mean()),
                "flags_or": int(np.bitwise_or.reduce(rec["flags"]))})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
