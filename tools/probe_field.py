#!/usr/bin/env python
"""Times the likelihood field on one MI355X.  Device events around `reps` back-to-back calls after a warm-up, three
rounds, the median round reported:

  field build   rr_rasterize_points_device of 16 clouds of about 4,800 points, and rr_distance_field_device at 1024 x 1024, max_dist 255
  scoring       rr_score_poses_device: 65,536 and 1,048,576 hypotheses of a 4,800-point scan on that field; hypotheses/s and look-ups/s
  baseline      the only way to score hypotheses without the field: rr_register_points_device with iterations = 0 on 4,096 copies of the
                scan against the map's cloud (nearest-point distance, not the same quantity: timed as the cost of the alternative)

Beside the scoring the model it is held against: look-ups * VALU operations per look-up (read from the ISA of k_field_score) at the chip's
fp32 vector issue rate.  Prints one JSON line.

    python tools/probe_field.py [--reps 5] [--only 65536]      (--only N: one hypothesis count in a loop, for a counter run under rocprofv3)
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radarays_ros_amd import native, params  # noqa: E402

# MI355X: 256 CUs x 4 SIMDs x 32 lanes, one fp32 VALU operation per lane and clock, 2.4 GHz
LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
# k_field_score's loop, per look-up (its ISA: about 525 instructions per step of 8 hypotheses, of which about 480 are VALU): the rotation
# (8), two subtractions and two IEEE divisions (div_scale x2, rcp, 5 fma, div_fmas, div_fixup: 11 each), four compares, two floors and
# conversions, the index and the 64-bit address, the selects and the three sums
VALU_PER_LOOKUP = 60
BYTES_PER_LOOKUP = 2      # the gather; a 64-byte line of the field holds 32 cells, a 4,800-point scan touches about 4,800 distinct lines


def timed(fn, stream, reps, sync):
    import torch
    for _ in range(2):
        fn()
    sync()
    rounds = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        rounds.append(e0.elapsed_time(e1) * 1e3 / reps)
    return {"median": round(sorted(rounds)[1], 1), "min": round(min(rounds), 1), "max": round(max(rounds), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=4800)
    ap.add_argument("--only", type=int, default=None)
    ap.add_argument("--baseline-copies", type=int, default=4096)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    A, P, SIDE = 400, a.points, 1024
    ctx = native.Context(0)
    ctx.set_config(params.kaist_preset(), A)
    g = native.field_config(SIDE, SIDE, 0.25, -128.0, -128.0, 255, 2)       # 256 m x 256 m at 0.25 m
    rs = np.random.RandomState(1)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)   # noqa: E731
    ptr = lambda t: t.data_ptr()   # noqa: E731

    def cloud(xy):
        p = np.zeros(len(xy), native.POINT_DTYPE)
        p["x"], p["y"] = xy[:, 0], xy[:, 1]
        return p

    def scan_xy():
        """a ring of walls seen from the sensor: consecutive points are neighbours in space, as in a detected scan"""
        th = np.sort(rs.uniform(0, 2 * np.pi, P))
        r = 40.0 + 25.0 * np.sin(3 * th) + rs.normal(0, 0.2, P)
        return np.stack([r * np.cos(th), r * np.sin(th)], -1)

    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    sync = lambda: ctx.synchronize(s)   # noqa: E731
    out = {"points": P, "grid": [SIDE, SIDE], "max_dist": 255, "reps": a.reps, "tiles": native.field_tile_sizes()}
    with torch.cuda.stream(stream):
        # ---- field build: 16 keyframes around the origin
        n_key = 16
        pts = np.zeros((n_key, P), native.POINT_DTYPE)
        offs = np.zeros((n_key, A + 1), np.uint32)
        key_states = native.se2_states(rs.uniform(-np.pi, np.pi, n_key), rs.uniform(-20, 20, n_key), rs.uniform(-20, 20, n_key))
        for f in range(n_key):
            pts[f] = cloud(scan_xy())
            offs[f, -1] = P
        d_pts, d_offs, d_st = up(pts), up(offs), up(key_states)
        d_occ = torch.zeros(SIDE * SIDE, dtype=torch.uint8, device=dev)
        d_fld = torch.zeros(SIDE * SIDE, dtype=torch.int16, device=dev)
        if not a.only:
            out["rasterize_16_clouds_us"] = timed(lambda: ctx.rasterize_points_device(ptr(d_pts), ptr(d_offs), n_key, P, g, ptr(d_occ), ptr(d_st), s),
                                                  stream, a.reps, sync)
            out["distance_field_us"] = timed(lambda: ctx.distance_field_device(ptr(d_occ), g, ptr(d_fld), 1, s), stream, a.reps, sync)
        else:
            ctx.rasterize_points_device(ptr(d_pts), ptr(d_offs), n_key, P, g, ptr(d_occ), ptr(d_st), s)
            ctx.distance_field_device(ptr(d_occ), g, ptr(d_fld), 1, s)
        sync()
        out["occupied_cells"] = int(d_occ.sum().item())

        # ---- scoring: a scan taken near keyframe 0, hypotheses scattered around its pose
        scan = cloud(scan_xy())
        d_scan, d_cnt = up(scan), up(np.array([P], np.uint32))
        out["scoring"] = {}
        for n in ([a.only] if a.only else [65536, 1048576]):
            yaw = key_states[0, 0:2]
            base_yaw = np.arctan2(yaw[1], yaw[0])
            hy = base_yaw + rs.uniform(-0.1, 0.1, n)
            st = np.stack([np.cos(hy), np.sin(hy), key_states[0, 2] + rs.uniform(-2, 2, n), key_states[0, 3] + rs.uniform(-2, 2, n)], -1).astype(np.float32)
            d_hyp = up(st)
            d_rec = torch.zeros(n * native.FIELD_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            us = timed(lambda: ctx.score_poses_device(ptr(d_scan), ptr(d_cnt), P, ptr(d_hyp), n, ptr(d_fld), g, ptr(d_rec), s), stream, a.reps, sync)
            rec = d_rec.cpu().numpy().view(native.FIELD_DTYPE)
            lookups = float(n) * P
            model_us = lookups * VALU_PER_LOOKUP / LANE_OPS_PER_S * 1e6
            out["scoring"][str(n)] = {
                "us_per_call": us, "hypotheses_per_s": round(n / (us["median"] * 1e-6)), "lookups_per_s": round(lookups / (us["median"] * 1e-6)),
                "gathered_GB_per_s": round(lookups * BYTES_PER_LOOKUP / (us["median"] * 1e-6) / 1e9, 1),
                "model_valu_us": round(model_us, 1), "measured_over_model": round(us["median"] / model_us, 2),
                "mean_n_in": float(rec["n_in"].mean()), "mean_n_hit": float(rec["n_hit"].mean()), "best_sum_d2": int(rec["sum_d2"].min()),
            }

        # ---- baseline: the scan replicated once per hypothesis, against the cloud of keyframe 0, iterations = 0
        if not a.only:
            nb = a.baseline_copies
            rep = np.tile(scan, (nb, 1))
            boffs = np.zeros((nb, A + 1), np.uint32)
            boffs[:, -1] = P
            d_rep, d_boffs = up(rep), up(boffs)
            d_tgt = up(pts[0])
            d_brec = torch.zeros(nb * native.ICP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            us = timed(lambda: ctx.register_points_device(ptr(d_rep), ptr(d_boffs), nb, P, ptr(d_tgt), ptr(d_cnt), P, ptr(d_brec), None, 2.0, 0, None, s),
                       stream, max(1, a.reps // 2), sync)
            per_hyp = us["median"] / nb
            ours = out["scoring"]["65536"]["us_per_call"]["median"] / 65536
            out["baseline_icp_0_iterations"] = {"copies": nb, "us_per_call": us, "us_per_hypothesis": round(per_hyp, 3),
                                                "field_us_per_hypothesis": round(ours, 5), "ratio": round(per_hyp / ours, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
