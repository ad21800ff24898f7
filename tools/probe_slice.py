#!/usr/bin/env python
"""Times rr_slice_mesh_device (rr_slice.hip) on the benchmark's 10M-triangle map (config 4) at a 2048 x 2048 grid of 0.2 m cells around the
benchmark's pose: once with a 1 m band at sensor height, once with a 1 m band that contains the room's floor -- the rasteriser's worst case,
because the two floor faces cover the whole grid and take the large path alone.

Device events around `--reps` back-to-back calls after `--warmup` calls.  Reported per band: milliseconds per call; the share of faces that
pass the z reject and the length of the large list, both COUNTED on the host with the definition's own f32 arithmetic (identity poses: the
posed corners are the rest corners; a face that the tree builder cut has several records, so the device's counts are a little higher); the
cells marked; and the achieved bytes per second over the record and vertex stream (48 B of record, 12 B of face indices and 36 B of corners
per record) against the HBM3E peak of 8 TB/s.  One JSON line; needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from radarays_ros_amd import native, scenes  # noqa: E402

HBM_PEAK = 8.0e12


def host_counts(scene, g, z_lo, z_hi, small_cells, chunk=1 << 20):
    """(faces that pass the z reject, faces whose candidate box has more than small_cells cells, faces with a box at all)"""
    v, f = scene["verts"], scene["faces"]
    cell, x0, y0 = np.float32(g.cell), np.float32(g.x0), np.float32(g.y0)
    passed = large = boxed = 0
    for a in range(0, len(f), chunk):
        t = v[f[a:a + chunk].reshape(-1)].reshape(-1, 3, 3)
        z = t[:, :, 2]
        keep = ~((z.max(1) < np.float32(z_lo)) | (z.min(1) > np.float32(z_hi)))
        passed += int(keep.sum())
        t = t[keep]
        u, w = (t[:, :, 0] - x0) / cell, (t[:, :, 1] - y0) / cell
        xlo, xhi = np.maximum(np.ceil(u.min(1)) - 1, 0), np.minimum(np.floor(u.max(1)), g.width - 1)
        ylo, yhi = np.maximum(np.ceil(w.min(1)) - 1, 0), np.minimum(np.floor(w.max(1)), g.height - 1)
        ok = (xlo <= xhi) & (ylo <= yhi)
        n = np.where(ok, (xhi - xlo + 1) * (yhi - ylo + 1), 0)
        boxed += int(ok.sum())
        large += int((n > small_cells).sum())
    return passed, large, boxed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=4)
    ap.add_argument("--side", type=int, default=2048)
    ap.add_argument("--cell", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("probe_slice.py needs a GPU")
    dev = "cuda:0"
    t0 = time.time()
    s = scenes.config_scene(a.config)
    t_scene = time.time() - t0
    ctx = native.Context(0)
    t0 = time.time()
    ctx.set_mesh(s["verts"], s["faces"], s["face_object_id"], builder="gpu")
    t_mesh = time.time() - t0
    half = 0.5 * a.side * a.cell
    g = native.field_config(a.side, a.side, a.cell, 1.0 - half, 1.5 - half, 255, 0)
    sensor = float(scenes.ground_height(1.0, 1.5)) + 2.0
    floor = float(s["verts"][:, 2].min())
    small, tile, group = native.slice_tile_sizes()
    info = ctx.bvh_info()
    out = {"config": a.config, "faces": int(len(s["faces"])), "records": int(info["n_tris"]), "grid": [a.side, a.side], "cell": a.cell,
           "reps": a.reps, "warmup": a.warmup, "tiles": [small, tile, group], "scene_s": round(t_scene, 2), "set_mesh_gpu_s": round(t_mesh, 3),
           "bands": []}
    stream_bytes = int(info["n_tris"]) * (48 + 12 + 36)
    cells = a.side * a.side
    for name, (lo, hi) in (("sensor height", (sensor - 0.5, sensor + 0.5)), ("floor", (floor - 0.5, floor + 0.5))):
        band = native.slice_config(lo, hi)
        d_occ = torch.zeros(cells, dtype=torch.uint8, device=dev)
        d_obj = torch.full((cells,), -1, dtype=torch.int32, device=dev)
        side = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        for _ in range(a.warmup):
            ctx.slice_mesh_device(band, g, d_occ.data_ptr(), d_obj.data_ptr(), None, side.cuda_stream)
        torch.cuda.synchronize()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            ev0.record()
            for _ in range(a.reps):
                ctx.slice_mesh_device(band, g, d_occ.data_ptr(), d_obj.data_ptr(), None, side.cuda_stream)
            ev1.record()
        torch.cuda.synchronize()
        ms = ev0.elapsed_time(ev1) / a.reps
        passed, large, boxed = host_counts(s, g, lo, hi, small)
        out["bands"].append({"band": name, "z_lo": round(lo, 3), "z_hi": round(hi, 3), "ms_per_call": round(ms, 4),
                             "faces_past_z_reject": passed, "share_past_z_reject": round(passed / len(s["faces"]), 6),
                             "faces_with_a_box": boxed, "large_list_faces": large, "cells_marked": int((d_occ != 0).sum().item()),
                             "stream_bytes": stream_bytes, "bytes_per_s": round(stream_bytes / (ms * 1e-3), 1),
                             "share_of_hbm_peak": round(stream_bytes / (ms * 1e-3) / HBM_PEAK, 4)})
    line = json.dumps(out)
    print(line)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
