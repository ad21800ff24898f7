#!/usr/bin/env python
"""Times the scan matcher on one MI355X: 16 and 64 clouds of about 4,800 points registered against a target
of 4,800 points by rr_register_points_device at 10 iterations.  Device events around `reps` back-to-back calls after a warm-up; the
time per (pass, solve) pair is the call at 10 iterations minus the call at 0 iterations, over 10: it holds k_icp_pass, k_icp_solve (one
thread per cloud) and the gap between the two launches.  Beside it the model the measurement is held against: distance evaluations * 8
VALU operations at the chip's fp32 vector issue rate (a wave64 instruction issues in 2 clocks on a 32-lane SIMD).  Prints one JSON line.

    python tools/probe_icp.py [--reps 10] [--only 64]      (--only N: one batch size in a loop, for a counter run under rocprofv3)
"""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radarays_ros_amd import native, params  # noqa: E402

# MI355X: 256 CUs x 4 SIMDs x 32 lanes, one fp32 VALU operation per lane and clock, 2.4 GHz (half the 157.3 TFLOPS peak, which counts
# an FMA as two).  One wave alone on a SIMD sustains half of that: 4 clocks per instruction, not 2
LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
OPS_PER_EVAL = 8      # 2 sub, 2 mul, 1 add, 1 compare, 2 selects (the ISA adds one v_mov of the index per target)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--points", type=int, default=4800)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--only", type=int, default=None)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    A, P, IT = 400, a.points, a.iterations
    ctx = native.Context(0)
    ctx.set_config(params.kaist_preset(), A)
    rs = np.random.RandomState(1)
    tgt_xy = rs.uniform(-100, 100, (P, 2))                                # about one point per 8 m^2: a CFAR cloud's density
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)   # noqa: E731

    def cloud(xy):
        p = np.zeros(len(xy), native.POINT_DTYPE)
        p["x"], p["y"] = xy[:, 0], xy[:, 1]
        return p

    d_tgt, d_cnt = up(cloud(tgt_xy)), up(np.array([P], np.uint32))
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    out = {"points": P, "target": P, "iterations": IT, "reps": a.reps, "tiles": native.icp_tile_sizes(), "batches": {}}
    for n in ([a.only] if a.only else [16, 64]):
        pts = np.zeros((n, P), native.POINT_DTYPE)
        offs = np.zeros((n, A + 1), np.uint32)
        for f in range(n):                                                # each cloud: the target seen from a pose 0.5 m and 2 degrees away, jittered
            m = P - rs.randint(0, 64)
            yaw, t = rs.uniform(-0.035, 0.035), rs.uniform(-0.5, 0.5, 2)
            q = tgt_xy[rs.permutation(P)[:m]] + rs.normal(0, 0.05, (m, 2)) - t
            c, sn = math.cos(yaw), math.sin(yaw)
            pts[f, :m] = cloud(np.stack([c * q[:, 0] + sn * q[:, 1], -sn * q[:, 0] + c * q[:, 1]], -1))
            offs[f, -1] = m
        d_pts, d_offs = up(pts), up(offs)
        d_rec = torch.zeros(n * native.ICP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        P_ = lambda t: t.data_ptr()   # noqa: E731
        us = {}
        with torch.cuda.stream(stream):
            for it in (0, IT):
                fn = lambda it=it: ctx.register_points_device(P_(d_pts), P_(d_offs), n, P, P_(d_tgt), P_(d_cnt), P, P_(d_rec), None, 2.0, it, None, s)   # noqa: E731
                for _ in range(2):
                    fn()
                ctx.synchronize(s)
                rounds = []
                for _ in range(3):                                        # three rounds of `reps` calls: the median round is reported
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(a.reps):
                        fn()
                    e1.record(stream)
                    e1.synchronize()
                    rounds.append(e0.elapsed_time(e1) * 1e3 / a.reps)
                us[it] = {"median": round(sorted(rounds)[1], 1), "min": round(min(rounds), 1), "max": round(max(rounds), 1)}
        rec = d_rec.cpu().numpy().view(native.ICP_DTYPE)
        evals = float(offs[:, -1].sum()) * P
        per_pass = (us[IT]["median"] - us[0]["median"]) / IT
        model_pass = evals * OPS_PER_EVAL / LANE_OPS_PER_S * 1e6
        out["batches"][str(n)] = {
            "us_per_call_0_iterations": us[0], "us_per_call": us[IT], "us_per_pass_solve_pair": round(per_pass, 1),
            "evaluations_per_pass": evals, "model_us_per_pass": round(model_pass, 1), "model_us_per_call": round(model_pass * (IT + 1), 1),
            "waves_per_pass": int(sum(2 * -(-int(m) // out["tiles"][0]) for m in offs[:, -1])),     # two waves per workgroup of 128 threads
            "measured_over_model": round(per_pass / model_pass, 2),
            "mean_matched": float(rec["n_matched"].mean()), "flags_or": int(np.bitwise_or.reduce(rec["flags"])),
        }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
