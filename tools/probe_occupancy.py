#!/usr/bin/env python
"""Times occupancy mapping on one MI355X.  Device events around `reps` back-to-back calls after a warm-up, three
rounds, the median round reported:

  update        rr_occupancy_update_device: 64 scans of about 4,800 points (400 azimuths x 12 detections) under 64 states into a
                1024 x 1024 evidence grid of 0.25 m cells -- the profile, cells x scans of the inverse sensor model, the hits
  map           rr_occupancy_map_device on that grid
  baseline      the same information through the only route there was before: rr_polar_to_cartesian_device (nearest) once per scan into a
                1024 x 1024 bird's-eye image in the scan's OWN frame -- what is occupied and what is empty around one pose; turning 64 such
                images into one map (a resampling per scan and a sum) would come on top and is not timed

Beside the update the model k_occ_free is held against: cells x scans x the VALU instructions per (cell, scan) counted in its ISA, at the
chip's fp32 vector issue rate.  Prints one JSON line.

    python tools/probe_occupancy.py [--reps 5] [--scans 64] [--only-update]      (--only-update: for a counter run under rocprofv3)
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
# k_occ_free's scan loop, per (cell, scan), from its ISA (hipcc -S, gfx950): about 410 VALU instructions per iteration of four cells when
# the loop inside fmodf is not entered -- atan2f with its IEEE division (68 per cell), the azimuth coordinate (a second IEEE division,
# fmodf, three range fix-ups, rintf: about 24 per cell), the rigid transform and rho2 (8), the address and the compare -- plus four
# f64-to-f32 conversions of the state per iteration.  A count, not a measurement
VALU_PER_CELL_SCAN = 105


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
    ap.add_argument("--scans", type=int, default=64)
    ap.add_argument("--per-azimuth", type=int, default=12)
    ap.add_argument("--only-update", action="store_true")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    A, SIDE, N, K = 400, 1024, a.scans, a.per_azimuth
    cfg = params.kaist_preset()
    ctx = native.Context(0)
    ctx.set_config(cfg, A)
    n_cells, res = cfg.n_cells, cfg.resolution
    g = native.field_config(SIDE, SIDE, 0.25, -128.0, -128.0)               # 256 m x 256 m at 0.25 m
    o = native.occupancy_config(3, 2, int(np.ceil(0.71 * g.cell / res)), n_cells, n_cells)
    rs = np.random.RandomState(1)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)   # noqa: E731
    ptr = lambda t: t.data_ptr()   # noqa: E731

    # scans of a ring of walls 40 +- 25 m out, K detections per azimuth from the wall outwards: sorted by column, then bin
    P = A * K
    pts = np.zeros((N, P), native.POINT_DTYPE)
    offs = np.tile(np.arange(A + 1, dtype=np.uint32) * K, (N, 1))
    col = np.repeat(np.arange(A), K)
    theta = (np.float32(0.0) + col.astype(np.float32) * np.float32(-2 * np.pi / A)).astype(np.float32)
    for f in range(N):
        wall = 40.0 + 25.0 * np.sin(3 * theta[::K] + rs.uniform(0, 2 * np.pi)) + rs.normal(0, 0.2, A)
        first = np.clip((wall / res).astype(np.int64), 1, n_cells - 9 * K - 1)
        b = (first[:, None] + np.sort(rs.choice(8 * K, (A, K)), axis=1) + np.arange(K)[None, :]).reshape(-1)   # strictly ascending per column
        r = ((b + 0.5) * res).astype(np.float32)
        pts[f]["x"], pts[f]["y"], pts[f]["intensity"], pts[f]["column"], pts[f]["bin"] = r * np.cos(theta), r * np.sin(theta), 100.0, col, b
    states = native.se2_states(rs.uniform(-np.pi, np.pi, N), rs.uniform(-20, 20, N), rs.uniform(-20, 20, N))

    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    sync = lambda: ctx.synchronize(s)   # noqa: E731
    out = {"scans": N, "points_per_scan": P, "grid": [SIDE, SIDE], "reps": a.reps, "tiles": native.occupancy_tile_sizes()}
    with torch.cuda.stream(stream):
        d_pts, d_offs, d_st = up(pts), up(offs), up(states)
        d_prof = torch.zeros(N * A, dtype=torch.float32, device=dev)
        d_ev = torch.zeros(SIDE * SIDE, dtype=torch.int32, device=dev)
        d_occ = torch.zeros(SIDE * SIDE, dtype=torch.uint8, device=dev)
        update = lambda: ctx.occupancy_update_device(ptr(d_pts), ptr(d_offs), N, P, g, o, ptr(d_prof), ptr(d_ev), ptr(d_st), s)   # noqa: E731
        us = timed(update, stream, a.reps, sync)
        pairs = float(SIDE) * SIDE * N
        model_us = pairs * VALU_PER_CELL_SCAN / LANE_OPS_PER_S * 1e6
        out["update_us"] = us
        out["cell_scans_per_s"] = round(pairs / (us["median"] * 1e-6))
        out["model_valu_us"] = round(model_us, 1)
        out["measured_over_model"] = round(us["median"] / model_us, 2)
        if not a.only_update:
            d_ev.zero_()
            update()
            out["map_us"] = timed(lambda: ctx.occupancy_map_device(ptr(d_ev), g, ptr(d_occ), s), stream, a.reps, sync)
            sync()
            occ = d_occ.cpu().numpy()
            out["cells"] = {"occupied": int((occ > 128).sum()), "free": int((occ < 128).sum()), "unknown": int((occ == 128).sum())}
            # ---- baseline: one bird's-eye image per scan, in the scan's own frame
            imgs = torch.zeros((1, n_cells, A), dtype=torch.uint8, device=dev)
            cart = torch.zeros((SIDE, SIDE), dtype=torch.uint8, device=dev)

            def per_scan():
                for _ in range(N):
                    ctx.polar_to_cartesian_device(ptr(imgs), 1, SIDE, g.cell, ptr(cart), False, s)
            base = timed(per_scan, stream, max(1, a.reps // 2), sync)
            out["baseline_cartesian_per_scan_us"] = base
            out["baseline_over_update"] = round(base["median"] / us["median"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
