#!/usr/bin/env python
"""Times the beam model on one MI355X.  Device events around `reps` back-to-back calls after a warm-up, three
rounds, the median round reported:

  score form    rr_score_beams_device: 65,536 and 1,048,576 hypotheses of 400 azimuths on a 1024 x 1024 field, around the most open spot of
                the map
  range form    rr_cast_map_device: 4,096 hypotheses of 400 azimuths on the same field
  context       the parent's rr_score_poses_device on the same hypotheses and a 4,800-point scan: a DIFFERENT quantity (one look-up per
                point where a ray takes as many as its march needs), recorded beside the beam model, not against it

The look-ups of a call are counted, not estimated: tests/cast_ref.py's skip_march, the rule as the kernel applies it, on a sample of the
hypotheses (so this tool imports the test tree's restatement, on purpose: the count is the restatement's own).  Beside the times the model they are held against: samples * VALU operations per sample (read from the ISA of k_cast) at the
chip's fp32 vector issue rate.  Prints one JSON line.

    python tools/probe_cast.py [--reps 5] [--only 65536]      (--only N: one hypothesis count of the score form in a loop, for a counter run)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from radarays_ros_amd import native, params  # noqa: E402

# MI355X: 256 CUs x 4 SIMDs x 32 lanes, one fp32 VALU operation per lane and clock, 2.4 GHz
LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
# k_cast's march loop, per sample (its ISA): 46 VALU instructions to the IN GRID test -- the bin's range through f64 (4, at half rate), the
# rotation, two IEEE divisions of 11 each -- and 38 more for an IN GRID sample: index, gather, the square root with its correction, the skip
VALU_PER_SAMPLE_OUT, VALU_PER_LOOKUP = 46, 86
BYTES_PER_LOOKUP = 2      # the gather


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
    ap.add_argument("--counted", type=int, default=64, help="hypotheses whose look-ups the restatement counts")
    a = ap.parse_args()
    import torch
    import cast_ref
    dev = torch.device("cuda", 0)
    A, P, SIDE = 400, a.points, 1024
    ctx = native.Context(0)
    cfg = params.kaist_preset()
    ctx.set_config(cfg, A)
    n_cells, res = int(cfg.n_cells), float(cfg.resolution)
    g = native.field_config(SIDE, SIDE, 0.25, -128.0, -128.0, 255, 8)       # 256 m x 256 m at 0.25 m
    beam = native.beam_config(0, n_cells, n_cells, 1, 6, 24)
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
    out = {"n_angles": A, "n_cells": n_cells, "resolution": res, "grid": [SIDE, SIDE], "max_dist": 255, "reps": a.reps, "tiles": native.cast_tile_sizes()}
    with torch.cuda.stream(stream):
        # ---- the map: 16 keyframes around the origin, rasterised, and its field
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
        ctx.rasterize_points_device(ptr(d_pts), ptr(d_offs), n_key, P, g, ptr(d_occ), ptr(d_st), s)
        ctx.distance_field_device(ptr(d_occ), g, ptr(d_fld), 1, s)
        sync()
        fld = d_fld.cpu().numpy().view(np.uint16).reshape(SIDE, SIDE)
        out["occupied_cells"] = int((fld == 0).sum())
        dirs = native.beam_directions(ctx._rrcfg)
        d_dirs = up(dirs)
        # the hypotheses stand where the map is most open within 20 m of the origin (the walls are 0.2 m of noise thick: a sensor inside one
        # would see 1 m far), within +-1 m and +-0.05 rad
        lo, hi = SIDE // 2 - 80, SIDE // 2 + 80
        iy, ix = np.unravel_index(int(np.argmax(fld[lo:hi, lo:hi])), (hi - lo, hi - lo))
        base_x, base_y, base_yaw = g.x0 + (lo + ix + 0.5) * g.cell, g.y0 + (lo + iy + 0.5) * g.cell, 0.3
        out["base"] = {"x": round(float(base_x), 3), "y": round(float(base_y), 3), "nearest_wall_m": round(float(np.sqrt(fld[lo + iy, lo + ix])) * g.cell, 2)}

        def hypotheses(n):
            st = native.se2_states(base_yaw + rs.uniform(-0.05, 0.05, n), base_x + rs.uniform(-1, 1, n), base_y + rs.uniform(-1, 1, n))
            return np.ascontiguousarray(st, np.float32)

        # ---- what the restatement counts on a sample of the hypotheses
        sample = hypotheses(a.counted)
        e, looks, visits = cast_ref.skip_march(sample, dirs, fld, g, beam, res)
        out["counted"] = {"hypotheses": a.counted, "lookups_per_ray": round(float(looks.mean()), 2), "samples_per_ray": round(float(visits.mean()), 2),
                          "brute_force_bins_per_ray": round(float(np.minimum(e.astype(np.int64) + 1, n_cells).mean()), 2),
                          "rays_that_hit": round(float((e < n_cells).mean()), 3)}
        first = np.minimum(e[0].astype(np.int64) + rs.randint(-8, 9, A), n_cells).clip(0).astype(np.uint16)
        d_first = up(first)

        def model(n):
            lookups, samples = n * A * looks.mean(), n * A * visits.mean()
            valu = lookups * VALU_PER_LOOKUP + (samples - lookups) * VALU_PER_SAMPLE_OUT
            return lookups, valu / LANE_OPS_PER_S * 1e6

        out["score"] = {}
        for n in ([a.only] if a.only else [65536, 1048576]):
            d_hyp = up(hypotheses(n))
            d_rec = torch.zeros(n * native.BEAM_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            reps = a.reps if n <= 65536 else max(1, a.reps // 2)
            us = timed(lambda: ctx.score_beams_device(ptr(d_first), ptr(d_hyp), n, ptr(d_dirs), ptr(d_fld), g, beam, ptr(d_rec), s), stream, reps, sync)
            rec = d_rec.cpu().numpy().view(native.BEAM_DTYPE)
            lookups, model_us = model(n)
            out["score"][str(n)] = {"us_per_call": us, "hypotheses_per_s": round(n / (us["median"] * 1e-6)), "rays_per_s": round(n * A / (us["median"] * 1e-6)),
                                    "lookups_per_s": round(lookups / (us["median"] * 1e-6)),
                                    "gathered_GB_per_s": round(lookups * BYTES_PER_LOOKUP / (us["median"] * 1e-6) / 1e9, 1),
                                    "model_valu_us": round(model_us, 1), "measured_over_model": round(us["median"] / model_us, 2),
                                    "mean_n_agree": float(rec["n_agree"].mean()), "mean_n_cast": float(rec["n_cast"].mean())}
        if not a.only:
            n = 4096
            d_hyp = up(hypotheses(n))
            d_rng = torch.zeros(n * A, dtype=torch.int16, device=dev)
            us = timed(lambda: ctx.cast_map_device(ptr(d_hyp), n, ptr(d_dirs), ptr(d_fld), g, beam, ptr(d_rng), s), stream, a.reps, sync)
            lookups, model_us = model(n)
            out["ranges"] = {str(n): {"us_per_call": us, "rays_per_s": round(n * A / (us["median"] * 1e-6)),
                                      "lookups_per_s": round(lookups / (us["median"] * 1e-6)), "model_valu_us": round(model_us, 1),
                                      "measured_over_model": round(us["median"] / model_us, 2)}}
            # ---- context, a different quantity: the likelihood field's scorer on the same hypotheses and a 4,800-point scan
            scan = cloud(scan_xy())
            d_scan, d_cnt = up(scan), up(np.array([P], np.uint32))
            out["context_score_poses"] = {}
            for n in (65536, 1048576):
                d_hyp = up(hypotheses(n))
                d_rec = torch.zeros(n * native.FIELD_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                reps = a.reps if n <= 65536 else max(1, a.reps // 2)
                us = timed(lambda: ctx.score_poses_device(ptr(d_scan), ptr(d_cnt), P, ptr(d_hyp), n, ptr(d_fld), g, ptr(d_rec), s), stream, reps, sync)
                out["context_score_poses"][str(n)] = {"us_per_call": us, "lookups_per_s": round(n * P / (us["median"] * 1e-6))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
