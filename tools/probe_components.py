#!/usr/bin/env python
"""Times connected-component labelling on one MI355X.  Device events around `reps` back-to-back calls of
rr_label_components_device after a warm-up, three rounds, the median round reported as ms per plane:

  polar     16 polar planes of 3424 x 400 from a simulated batch of the box room (tests/icp_ref.py's scene, so this tool imports the test
            tree on purpose), thresholded, wrap_x on, labels and records
  sparse    one 4096 x 4096 occupancy map at a density of about 0.05, labels, cleaned plane and records, min_pixels 3
  dense     one such map at 0.45: beyond the 8-connectivity percolation threshold, so one record takes most pixels -- the contended case

Beside each the floor any labeller has: one plain pass over the same planes that reads the uint8 plane and writes a uint32 plane, run as a
small kernel of its own (torch's element-wise conversion kernel, timed the same way), and the time of scipy.ndimage.label on the same
planes on the host where scipy imports.  Prints one JSON line.

    python tools/probe_components.py [--reps 5] [--no-scipy]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from radarays_ros_amd import native, params, radar  # noqa: E402


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
        rounds.append(e0.elapsed_time(e1) / reps)
    return sorted(rounds)[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    import torch
    import icp_ref
    from common import golden_beams
    dev = torch.device("cuda", 0)
    s = icp_ref.loop_scene()
    r = radar.RadarHIP(s["verts"], s["faces"], s["face_object_id"])
    r.loadParams(params.kaist_materials(), s["object_materials"], 0)
    r.updateDynCfg(params.kaist_preset(n_samples=icp_ref.LOOP_SAMPLES))
    r.setBeamSamples(golden_beams(icp_ref.LOOP_SAMPLES))
    r._push()
    ctx = r._ctx
    n_cells = int(r.m_cfg.n_cells)
    poses = native.object_poses_array(np.stack([icp_ref.loop_pose((0.3 * k - 2.0, 0.1 * k, 0.05 * k)) for k in range(16)]))
    polar = torch.empty((16, n_cells, radar.N_ANGLES), dtype=torch.uint8, device=dev)
    ctx.simulate_batch_device(poses, polar.data_ptr(), None)
    ctx.synchronize()
    rs = np.random.default_rng(5)
    maps = {d: torch.from_numpy((rs.random((1, 4096, 4096)) < d).astype(np.uint8) * 200).to(dev) for d in (0.05, 0.45)}
    work = [("polar", polar, native.components_config(n_cells, radar.N_ANGLES, 20, 8, True, 1, 4096), True, False),
            ("sparse", maps[0.05], native.components_config(4096, 4096, 129, 8, False, 3, 1 << 20), True, True),
            ("dense", maps[0.45], native.components_config(4096, 4096, 129, 8, False, 3, 1 << 20), True, True)]
    stream = torch.cuda.Stream(device=dev)
    sync = lambda: ctx.synchronize(stream.cuda_stream)       # noqa: E731
    out = {"reps": a.reps}
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        for name, planes, g, labels, clean in work:
            n, npx = int(planes.shape[0]), g.height * g.width
            bufs = ctx.label_components_tensors(planes, g, labels, clean, stream.cuda_stream)
            sync()
            ptr = lambda k: bufs[k].data_ptr() if k in bufs else None      # noqa: E731
            call = lambda: ctx.label_components_device(planes.data_ptr(), n, g, ptr("labels"), ptr("clean"), ptr("comps"), ptr("counts"),   # noqa: E731
                                                       ptr("scratch"), bufs["scratch"].numel(), stream.cuda_stream)
            ms = timed(call, stream, a.reps, sync)
            u32 = torch.empty(planes.shape, dtype=torch.int32, device=dev)
            floor = timed(lambda: u32.copy_(planes), stream, a.reps, sync)
            counts = native.Context.component_counts(bufs["counts"])
            row = {"planes": n, "pixels_per_plane": npx, "foreground": round(float((planes >= g.threshold).float().mean().item()), 4),
                   "kept": counts[:, 0].tolist() if n == 1 else int(counts[:, 0].sum()), "dropped": int(counts[:, 1].sum()),
                   "ms_per_plane": round(ms / n, 4), "floor_ms_per_plane": round(floor / n, 4), "ratio_to_floor": round(ms / floor, 1),
                   "scratch_mib": round(bufs["scratch"].numel() / 2.0 ** 20, 1)}
            if not a.no_scipy:
                try:
                    from scipy import ndimage
                    host = planes.cpu().numpy() >= g.threshold
                    t0 = time.perf_counter()
                    for p in host[:2]:
                        ndimage.label(p, structure=np.ones((3, 3), int))
                    row["scipy_ms_per_plane"] = round((time.perf_counter() - t0) * 1e3 / len(host[:2]), 1)
                except ImportError:
                    pass
            out[name] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
