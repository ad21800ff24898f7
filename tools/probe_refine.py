#!/usr/bin/env python
"""Times map refinement on one MI355X.  Device events around `reps` back-to-back calls after a warm-up, three
rounds, the median round reported:

  transform     rr_nearest_field_device at 1024 x 1024, max_dist 255, beside rr_distance_field_device on the same map in the same run
  refinement    rr_refine_poses_device: 4,096, 65,536 and 1,048,576 hypotheses of a 4,800-point scan against that table, 10 iterations
                (11 passes); hypotheses/s and look-ups/s
  alternative   the parent's only route to a refined pose: rr_register_points_device with the map's occupied cell centres as the target, on
                as many copies of the scan as fit its limits (a near but not identical quantity: timed as the cost of the alternative)

Beside the refinement the model it is held against: look-ups * VALU operations per look-up (read from the ISA of k_refine) at the chip's
fp32 vector issue rate.  Prints one JSON line.

    python tools/probe_refine.py [--reps 5] [--only 65536]      (--only N: one hypothesis count in a loop, for a counter run under rocprofv3)
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
# k_refine's point loop, per look-up (its ISA: one step of 4 hypotheses is about 250 VALU instructions of rotation, cell rule -- two IEEE
# divisions of 11 each --, address and gather, and 62 per hypothesis of index split, quantisation and the eight 64-bit sums): (250 + 3 * 62) / 4
VALU_PER_LOOKUP = 109
BYTES_PER_LOOKUP = 4      # the gather


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
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--only", type=int, default=None)
    ap.add_argument("--alternative-copies", type=int, default=64)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    A, P, SIDE, IT = 400, a.points, 1024, a.iterations
    ctx = native.Context(0)
    ctx.set_config(params.kaist_preset(), A)
    g = native.field_config(SIDE, SIDE, 0.25, -128.0, -128.0, 255, 8)       # 256 m x 256 m at 0.25 m, a gate of 2 m
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
    out = {"points": P, "grid": [SIDE, SIDE], "max_dist": 255, "iterations": IT, "reps": a.reps, "tiles": native.refine_tile_sizes()}
    with torch.cuda.stream(stream):
        # ---- the map: 16 keyframes around the origin, rasterised
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
        d_near = torch.zeros(SIDE * SIDE, dtype=torch.int32, device=dev)
        ctx.rasterize_points_device(ptr(d_pts), ptr(d_offs), n_key, P, g, ptr(d_occ), ptr(d_st), s)
        sync()
        if not a.only:
            out["nearest_field_us"] = timed(lambda: ctx.nearest_field_device(ptr(d_occ), g, ptr(d_near), 1, s), stream, a.reps, sync)
            out["distance_field_us"] = timed(lambda: ctx.distance_field_device(ptr(d_occ), g, ptr(d_fld), 1, s), stream, a.reps, sync)
        else:
            ctx.nearest_field_device(ptr(d_occ), g, ptr(d_near), 1, s)
        sync()
        occ = d_occ.cpu().numpy()
        out["occupied_cells"] = int(occ.sum())

        # ---- refinement: a scan taken near keyframe 0, hypotheses scattered around its pose
        scan = cloud(scan_xy())
        d_scan, d_cnt = up(scan), up(np.array([P], np.uint32))
        base_yaw = np.arctan2(key_states[0, 1], key_states[0, 0])
        out["refinement"] = {}
        for n in ([a.only] if a.only else [4096, 65536, 1048576]):
            st = native.se2_states(base_yaw + rs.uniform(-0.05, 0.05, n), key_states[0, 2] + rs.uniform(-1, 1, n), key_states[0, 3] + rs.uniform(-1, 1, n))
            d_hyp = up(st)
            d_rec = torch.zeros(n * native.ICP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            reps = a.reps if n <= 65536 else max(1, a.reps // 2)
            us = timed(lambda: ctx.refine_poses_device(ptr(d_scan), ptr(d_cnt), P, ptr(d_hyp), n, ptr(d_near), g, ptr(d_rec), IT, s), stream, reps, sync)
            rec = d_rec.cpu().numpy().view(native.ICP_DTYPE)
            lookups = float(n) * P * (IT + 1)
            model_us = lookups * VALU_PER_LOOKUP / LANE_OPS_PER_S * 1e6
            out["refinement"][str(n)] = {
                "us_per_call": us, "hypotheses_per_s": round(n / (us["median"] * 1e-6)), "lookups_per_s": round(lookups / (us["median"] * 1e-6)),
                "gathered_GB_per_s": round(lookups * BYTES_PER_LOOKUP / (us["median"] * 1e-6) / 1e9, 1),
                "model_valu_us": round(model_us, 1), "measured_over_model": round(us["median"] / model_us, 2),
                "mean_n_matched": float(rec["n_matched"].mean()), "degenerate": int((rec["flags"] & native.ICP_DEGENERATE != 0).sum()),
                "median_rms_m": float(np.median(np.sqrt(rec["sse"] / np.maximum(rec["n_matched"], 1)) / 256.0)),
            }

        # ---- the alternative: the scan replicated once per hypothesis, against the occupied cells' centres (cut at the matcher's 65,536)
        if not a.only:
            nb = a.alternative_copies
            jy, jx = np.divmod(np.nonzero(occ)[0][:native.ICP_MAX_POINTS].astype(np.int64), SIDE)
            centres = np.stack([g.x0 + (jx + 0.5) * g.cell, g.y0 + (jy + 0.5) * g.cell], -1).astype(np.float32)
            T = len(centres)
            rep = np.tile(scan, (nb, 1))
            boffs = np.zeros((nb, A + 1), np.uint32)
            boffs[:, -1] = P
            init = native.se2_states(base_yaw + rs.uniform(-0.05, 0.05, nb), key_states[0, 2] + rs.uniform(-1, 1, nb), key_states[0, 3] + rs.uniform(-1, 1, nb))
            d_rep, d_boffs, d_tgt, d_tcnt, d_init = up(rep), up(boffs), up(cloud(centres)), up(np.array([T], np.uint32)), up(init)
            d_brec = torch.zeros(nb * native.ICP_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            us = timed(lambda: ctx.register_points_device(ptr(d_rep), ptr(d_boffs), nb, P, ptr(d_tgt), ptr(d_tcnt), T, ptr(d_brec), ptr(d_init), 2.0, IT,
                                                          None, s), stream, max(1, a.reps // 2), sync)
            per_hyp = us["median"] / nb
            ours = out["refinement"]["65536"]["us_per_call"]["median"] / 65536
            out["alternative_register_points"] = {"copies": nb, "target_points": T, "launches": 2 * IT + 3, "us_per_call": us,
                                                  "us_per_hypothesis": round(per_hyp, 3), "refine_us_per_hypothesis": round(ours, 5),
                                                  "ratio": round(per_hyp / ours, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
