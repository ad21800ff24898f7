#!/usr/bin/env python
"""Times the particle filter step on one MI355X.  Device events around `reps` back-to-back calls after a warm-up,
three rounds, the median round reported, at n = 65,536 and 1,048,576 particles:

  resample      rr_filter_resample_device: n records -> cum, n ancestors, the summary (six launches)
  move          rr_filter_move_device: n states through the ancestors
  score         rr_score_poses_device on the same particles: a 4,800-point scan on a 1024 x 1024 field, as BASELINE.md section 20
  host route    what a filter had to do before: the records to the host, the numpy restatement of resample and move, the states back

The condition of the step: resample + move take less time than the scoring call at the same n, in the same run.  Beside the times the
bytes model -- 16 B of records read twice, 8 B of cum written and read, 32 B of states and 8 B of ancestors per particle -- and the
measured multiple of it at the chip's HBM rate.  Prints one JSON line.

    python tools/probe_filter.py [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from radarays_ros_amd import native, params  # noqa: E402

HBM_BYTES_PER_S = 8.0e12                       # MI355X: 8 TB/s peak
MODEL_BYTES_PER_PARTICLE = 2 * 16 + 2 * 8 + 32 + 8


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
    a = ap.parse_args()
    import torch
    import filter_ref as R
    dev = torch.device("cuda", 0)
    P, SIDE = a.points, 1024
    c = native.Context(0)
    c.set_config(params.kaist_preset(n_cells=3360), 400)
    rs = np.random.RandomState(1)
    cfg = native.field_config(SIDE, SIDE, 0.25, -128.0, -128.0, 255, 2)
    occ = (rs.random_sample((SIDE, SIDE)) < 0.005).astype(np.uint8)
    pts = np.zeros(P, native.POINT_DTYPE)
    ang, rad = rs.uniform(-np.pi, np.pi, P), rs.uniform(5.0, 100.0, P)
    pts["x"], pts["y"] = rad * np.cos(ang), rad * np.sin(ang)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    sync = lambda: torch.cuda.synchronize(dev)                          # noqa: E731
    QUANTUM, N_TABLE = 64, 4096
    table = native.filter_weight_table(60.0, QUANTUM, N_TABLE)
    out = {"points": P, "field": [SIDE, SIDE], "model_bytes_per_particle": MODEL_BYTES_PER_PARTICLE, "tile_sizes": native.filter_tile_sizes()}
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        d_occ = torch.from_numpy(occ).to(dev)
        d_field = torch.empty((SIDE, SIDE), dtype=torch.int16, device=dev)
        c.distance_field_device(d_occ.data_ptr(), cfg, d_field.data_ptr(), 1, s)
        d_pts = torch.from_numpy(pts.view(np.uint8)).to(dev)
        d_count = torch.tensor([P], dtype=torch.int32, device=dev)
        d_table = torch.from_numpy(table.view(np.int16)).to(dev)
        for n in (65536, 1 << 20):
            yaw = rs.uniform(-np.pi, np.pi, n)
            st = np.stack([np.cos(yaw), np.sin(yaw), rs.uniform(-20, 20, n), rs.uniform(-20, 20, n)], axis=1).astype(np.float32)
            d_st, d_out = torch.from_numpy(st).to(dev), torch.empty((n, 4), dtype=torch.float32, device=dev)
            d_recs = torch.empty((n, 2), dtype=torch.int64, device=dev)
            d_cum, d_anc = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
            d_sum = torch.empty(4, dtype=torch.int64, device=dev)
            fc = native.filter_config(0.05, np.radians(0.5), QUANTUM, N_TABLE, 12345, 1, 2)
            score = lambda: c.score_poses_device(d_pts.data_ptr(), d_count.data_ptr(), P, d_st.data_ptr(), n, d_field.data_ptr(), cfg,  # noqa: E731
                                                 d_recs.data_ptr(), s)
            resample = lambda: c.filter_resample_device(d_recs.data_ptr(), n, d_table.data_ptr(), n, fc, d_cum.data_ptr(),              # noqa: E731
                                                        d_anc.data_ptr(), d_sum.data_ptr(), s)
            move = lambda: c.filter_move_device(d_st.data_ptr(), n, d_anc.data_ptr(), n, (1.0, 0.0, 0.1, 0.0), fc, d_out.data_ptr(), s)  # noqa: E731
            row = {"score_us": timed(score, stream, a.reps, sync), "resample_us": timed(resample, stream, a.reps, sync),
                   "move_us": timed(move, stream, a.reps, sync)}
            sync()
            summary = d_sum.cpu().numpy().view(native.FILTER_SUMMARY_DTYPE)[0]
            row["n_unique"], row["n_eff"] = int(summary["n_unique"]), round(int(summary["total_weight"]) ** 2 / max(1, int(summary["sum_w2"])))
            # the host route: D2H of the records, the restatement, H2D of the states (the median of three)
            host = []
            for _ in range(3):
                sync()
                t0 = time.perf_counter()
                recs = d_recs.cpu().numpy().view(native.FIELD_DTYPE).reshape(-1)
                t1 = time.perf_counter()
                _, anc, _ = R.resample(recs["sum_d2"], table, QUANTUM, 12345, n)
                new = R.move(st, anc, (1.0, 0.0, 0.1, 0.0), fc.sigma_xy, fc.sigma_t, 1, 2)
                t2 = time.perf_counter()
                d_out.copy_(torch.from_numpy(new))
                sync()
                host.append((time.perf_counter() - t0, t1 - t0, t2 - t1))
            tot, d2h, work = sorted(host)[1]
            row["host_route_us"] = {"total": round(tot * 1e6), "d2h": round(d2h * 1e6), "numpy": round(work * 1e6), "h2d": round((tot - d2h - work) * 1e6)}
            step = row["resample_us"]["median"] + row["move_us"]["median"]
            row["step_us"] = round(step, 1)
            row["step_below_score"] = bool(step < row["score_us"]["median"])
            row["host_over_step"] = round(tot * 1e6 / step, 1)
            row["multiple_of_bytes_model"] = round(step * 1e-6 / (n * MODEL_BYTES_PER_PARTICLE / HBM_BYTES_PER_S), 1)
            out[str(n)] = row
    print(json.dumps(out))
    return 0 if all(out[str(n)]["step_below_score"] for n in (65536, 1 << 20)) else 1


if __name__ == "__main__":
    sys.exit(main())
