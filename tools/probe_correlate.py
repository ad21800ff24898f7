#!/usr/bin/env python
"""Times correlative scan matching on one MI355X.  Device events around `reps` back-to-back calls after a warm-up,
three rounds, the median round reported:

  pyramid       rr_field_pyramid_device of a 1024 x 1024 field, 8 levels
  search        rr_correlate_scan_device: a 4,800-point scan, 64 yaws, +-255 cells (16,711,744 nodes) at each of --levels, with the
                record's per-level `evaluated` and `kept`; levels 0 is the exhaustive search in the same code
  dense         rr_score_poses_device on the same node count in calls of 2^22 hypotheses: the lattice the search replaces

Every search must name the same winner.  Prints one JSON line.

    python tools/probe_correlate.py [--reps 3] [--levels 0,3,4,5,6] [--half 255] [--yaws 64]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radarays_ros_amd import native, params  # noqa: E402


def timed(fn, stream, reps, sync):
    import torch
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--points", type=int, default=4800)
    ap.add_argument("--levels", default="0,3,4,5,6")
    ap.add_argument("--half", type=int, default=255)
    ap.add_argument("--yaws", type=int, default=64)
    ap.add_argument("--capacity", type=int, default=1 << 20)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    A, P, SIDE = 400, a.points, 1024
    ctx = native.Context(0)
    ctx.set_config(params.kaist_preset(), A)
    g = native.field_config(SIDE, SIDE, 0.25, -128.0, -128.0, 255, 2)       # 256 m x 256 m at 0.25 m, as tools/probe_field.py
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
    n_nodes = a.yaws * (2 * a.half + 1) ** 2
    out = {"points": P, "grid": [SIDE, SIDE], "yaws": a.yaws, "half": a.half, "nodes": n_nodes, "reps": a.reps, "tiles": native.correlate_tile_sizes()}
    with torch.cuda.stream(stream):
        # the map: one keyframe at (3, -2, 0.3); the scan is the same walls seen again, so the winner is known: that pose
        walls = scan_xy()
        key = native.se2_states(0.3, 3.0, -2.0)
        offs = np.zeros((1, A + 1), np.uint32)
        offs[0, -1] = P
        d_pts, d_offs, d_st = up(cloud(walls)), up(offs), up(key)
        d_occ = torch.zeros(SIDE * SIDE, dtype=torch.uint8, device=dev)
        d_pyr = torch.zeros(9 * SIDE * SIDE, dtype=torch.int16, device=dev)
        ctx.rasterize_points_device(ptr(d_pts), ptr(d_offs), 1, P, g, ptr(d_occ), ptr(d_st), s)
        ctx.distance_field_device(ptr(d_occ), g, ptr(d_pyr), 1, s)            # plane 0, in place
        out["pyramid_8_levels_us"] = timed(lambda: ctx.field_pyramid_device(ptr(d_pyr), g, 8, ptr(d_pyr), s), stream, a.reps, sync)

        # the coarse candidate: 20 m and 0.2 rad off; the window of +-half cells and the yaws must hold the truth
        yaws = 0.3 + 0.2 + np.linspace(-0.4, 0.4, a.yaws)
        centre = (3.0 + 14.0, -2.0 - 14.0)
        d_scan, d_cnt = up(cloud(walls + rs.normal(0, 0.05, walls.shape))), up(np.array([P], np.uint32))
        d_rot = up(native.se2_states(yaws, *centre).astype(np.float32))
        d_rec = torch.zeros(native.CORR_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        out["search"], winners = {}, set()
        for levels in [int(v) for v in a.levels.split(",")]:
            k = native.corr_config(a.half, a.half, levels, a.capacity)
            nbytes = ctx.correlate_scratch_bytes(a.yaws, P, k)
            d_scr = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            us = timed(lambda: ctx.correlate_scan_device(ptr(d_scan), ptr(d_cnt), P, ptr(d_rot), a.yaws, ptr(d_pyr), g, k, ptr(d_rec), ptr(d_scr), nbytes, s),
                       stream, a.reps if levels else 1, sync)
            rec = d_rec.cpu().numpy().view(native.CORR_DTYPE)[0]
            winners.add((int(rec["rot"]), int(rec["dx"]), int(rec["dy"]), int(rec["sum_d2"])))
            out["search"][str(levels)] = {"us_per_call": us, "evaluated": rec["evaluated"][:levels + 1].tolist(), "kept": rec["kept"][:levels + 1].tolist(),
                                          "evaluated_total": int(rec["evaluated"].sum()), "flags": int(rec["flags"]), "upper": int(rec["upper"]),
                                          "sum_d2": int(rec["sum_d2"]), "n_hit": int(rec["n_hit"]), "scratch_bytes": nbytes}
        out["winner"] = sorted(winners)
        out["one_winner"] = len(winners) == 1

        # the dense lattice on the same node count: calls of 2^22 hypotheses (the states' values do not change the cost)
        n_call = 1 << 22
        calls = -(-n_nodes // n_call)
        hy = rs.uniform(yaws[0], yaws[-1], n_call)
        st = np.stack([np.cos(hy), np.sin(hy), centre[0] + rs.uniform(-60, 60, n_call), centre[1] + rs.uniform(-60, 60, n_call)], -1).astype(np.float32)
        d_hyp = up(st)
        d_recs = torch.zeros(n_call * native.FIELD_DTYPE.itemsize, dtype=torch.uint8, device=dev)

        def dense():
            for _ in range(calls):
                ctx.score_poses_device(ptr(d_scan), ptr(d_cnt), P, ptr(d_hyp), n_call, ptr(d_pyr), g, ptr(d_recs), s)
        out["dense_lattice"] = {"calls": calls, "hypotheses_per_call": n_call, "us_total": timed(dense, stream, 1, sync)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
