"""Echo provenance on the card: what rr_simulate_batch_provenance_device costs beside rr_simulate_batch_device on
the same workload, and its two kernels alone.

    python tools/probe_labels.py [--workloads config2,target] [--frames 8] [--reps 30] [--rounds 3] [--json out.json]

Per workload (bench.py's: config 2 = 100k triangles, 1 pass; target = 10M triangles, 4 passes; 400 azimuths x 200 beam samples,
ambient noise 2), batches of --frames poses from the 16-pose trajectory into device buffers:
1. images/s of the plain batch, of the provenance call with the label plane only, and with every output (labels, faces, echo
   stream with a stride of the lane's list capacity, counts): a host clock around --reps calls and one synchronise.  The three
   routes are alternated inside each round; the median over the rounds is reported.  The plain batches replay their launch graph,
   the provenance chains are issued kernel by kernel: that difference is part of the figure.
2. k_echo_gather and k_label alone: the context's kernel timer ("gather", "label") over the provenance calls of one more round in
   timing mode, microseconds per launch.
Before anything is timed the provenance call's images are compared with the plain batch's.  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from radarays_ros_amd import native, params, scenes  # noqa: E402
from radarays_ros_amd.fixtures import golden_beams, materials_for  # noqa: E402

WORKLOADS = {"config2": (2, 1, 200), "target": (4, 4, 200)}          # scene config, passes, beam samples (bench.py: WORKLOADS)
DEV = "cuda:0"


def rate(fn, reps, frames):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for k in range(reps):
        fn(k)
    torch.cuda.synchronize()
    return reps * frames / (time.perf_counter() - t)


def probe(name, frames, reps, rounds):
    scene_id, passes, n_beam = WORKLOADS[name]
    s = scenes.config_scene(scene_id)
    cfg = params.kaist_preset(n_reflections=passes, ambient_noise=2)
    c = native.Context(0)
    c.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    c.set_materials(materials_for(s), s["object_materials"], 0)
    c.set_config(cfg)
    c.set_beam_samples(golden_beams(n_beam))
    c.set_noise_offsets((np.random.RandomState(7).uniform(0, 1, 400) * 1000).astype(np.float32))
    traj = np.stack(scenes.trajectory(16, s["name"]))
    batch = lambda k: traj[(np.arange(frames) + k * frames) % 16]   # noqa: E731
    cap = n_beam * (2 ** (passes - 1))
    stride = sum(min(n_beam << p, cap) for p in range(passes)) + cap          # the lane's list capacity (no multipath echoes)
    img = torch.zeros((frames, cfg.n_cells, 400), dtype=torch.uint8, device=DEV)
    img2 = torch.zeros_like(img)
    lab = torch.zeros((frames, cfg.n_cells, 400), dtype=torch.int32, device=DEV)
    fac = torch.zeros_like(lab)
    ech = torch.zeros((frames * 400 * stride * 16,), dtype=torch.uint8, device=DEV)
    cnt = torch.zeros((frames, 400), dtype=torch.int32, device=DEV)
    routes = {
        "plain": lambda k: c.simulate_batch_device(batch(k), img.data_ptr()),
        "labels_only": lambda k: c.simulate_batch_provenance_device(batch(k), img2.data_ptr(), lab.data_ptr()),
        "all_outputs": lambda k: c.simulate_batch_provenance_device(batch(k), img2.data_ptr(), lab.data_ptr(), fac.data_ptr(), ech.data_ptr(), stride,
                                                                    cnt.data_ptr()),
    }
    routes["plain"](0); routes["all_outputs"](0)
    c.synchronize()
    same = bool(torch.equal(img, img2))
    counts = cnt.cpu().numpy()
    labelled = float((lab.cpu().numpy().view(np.uint32) != native.LABEL_NONE).mean())
    for fn in routes.values():          # warm-up: lanes, launch graphs, trace-row history
        for k in range(8):
            fn(k)
    samples = {r: [] for r in routes}
    for _ in range(rounds):
        for r, fn in routes.items():
            samples[r].append(rate(fn, reps, frames))
    out = {"frames_per_call": frames, "images_equal_plain": same, "echoes_per_azimuth_mean": float(counts.mean()), "echoes_per_azimuth_max": int(counts.max()),
           "echo_stride": stride, "labelled_pixel_share": labelled}
    for r in routes:
        out["images_per_s_" + r] = float(np.median(samples[r]))
    c.synchronize()
    c.set_timing_mode(1)
    for k in range(max(4, reps // 4)):
        routes["all_outputs"](k)
    c.synchronize()
    for kern in ("gather", "label", "shade", "column"):
        ms, n = c.kernel_time(kern, True)
        out["us_per_launch_" + kern] = 1e3 * ms / n if n else None
        out["launches_" + kern] = int(n)
    c.set_timing_mode(0)
    c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="config2,target")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = {"tool": "probe_labels", "device": torch.cuda.get_device_name(0)}
    for w in a.workloads.split(","):
        res[w] = probe(w, a.frames, a.reps, a.rounds)
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
