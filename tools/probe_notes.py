"""Object annotations on the card: what one record per object costs when the label planes stay on the GPU, against
reducing them on the host.

    python tools/probe_notes.py [--frames 16] [--reps 20] [--host-reps 2] [--rounds 3] [--json out.json]

On bench.py's config 2 (100k triangles, 1 pass, 400 azimuths x 200 beam samples, 3424 cells, ambient noise 2), batches of --frames
poses from the 16-pose trajectory:
1. images/s of two generation loops that both end with NOTE_DTYPE records on the host:
   "device": rr_simulate_batch_annotations (provenance chain, annotation, records down);
   "host":   rr_simulate_batch_provenance_device, the label planes and images copied to the host, tests/notes_ref.py on them.
   A host clock around the calls; the loops are alternated inside each round, the median over the rounds is reported.
2. the records of the two loops are compared before anything is timed (integers bit for bit).
3. run under `rocprofv3 --kernel-trace --stats -- python tools/probe_notes.py`, the trace holds k_note_init / k_note_accum /
   k_note_finish of --frames frames; the time reading the planes once at HBM rate would take is printed beside them.
One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import notes_ref  # noqa: E402
from radarays_ros_amd import native, params, scenes  # noqa: E402
from radarays_ros_amd.fixtures import golden_beams, materials_for  # noqa: E402

DEV = "cuda:0"
HBM_BYTES_PER_S = 8.0e12          # the card's peak; what a streaming read reaches is below it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--mask", type=int, default=native.NOTE_DIRECT)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    frames = a.frames
    s = scenes.config_scene(2)
    cfg = params.kaist_preset(n_reflections=1, ambient_noise=2)
    c = native.Context(0)
    c.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    c.set_materials(materials_for(s), s["object_materials"], 0)
    c.set_config(cfg)
    c.set_beam_samples(golden_beams(200))
    c.set_noise_offsets((np.random.RandomState(7).uniform(0, 1, 400) * 1000).astype(np.float32))
    traj = np.stack(scenes.trajectory(16, s["name"]))
    batch = lambda k: traj[(np.arange(frames) + k * frames) % 16]   # noqa: E731
    g = c._rrcfg
    geo = dict(scroll=g.scroll_image, theta_min=g.theta_min, theta_inc=g.theta_inc, resolution=g.resolution)
    img = torch.zeros((frames, cfg.n_cells, 400), dtype=torch.uint8, device=DEV)
    lab = torch.zeros((frames, cfg.n_cells, 400), dtype=torch.int32, device=DEV)

    def device_loop(k):
        return c.simulate_batch_annotations(batch(k), a.mask)[0]

    def host_loop(k):
        c.simulate_batch_provenance_device(batch(k), img.data_ptr(), lab.data_ptr())
        c.synchronize()
        return notes_ref.annotate(lab.cpu().numpy().view(np.uint32), img.cpu().numpy(), c.n_objects, a.mask, **geo)[0]

    def rate(fn, reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for k in range(reps):
            fn(k)
        torch.cuda.synchronize()
        return reps * frames / (time.perf_counter() - t)

    dev, ref = device_loop(0), host_loop(0)
    same = all(np.array_equal(dev[k], ref[k]) for k in notes_ref.INT_FIELDS)
    for k in range(4):                                   # warm-up: lanes, buffers, trace-row history
        device_loop(k)
    samples = {"device": [], "host": []}
    for _ in range(a.rounds):
        samples["device"].append(rate(device_loop, a.reps))
        samples["host"].append(rate(host_loop, a.host_reps))
    plane_bytes = frames * cfg.n_cells * 400 * 5          # labels and image, read once
    res = {"tool": "probe_notes", "device": torch.cuda.get_device_name(0), "frames_per_call": frames, "n_objects": int(c.n_objects),
           "extent_mask": a.mask, "records_equal": bool(same),
           "labelled_pixel_share": float((lab.cpu().numpy().view(np.uint32) != native.LABEL_NONE).mean()),
           "visible_objects_mean": float((dev["n_direct"] > 0).sum(axis=1).mean()),
           "images_per_s_device": float(np.median(samples["device"])), "images_per_s_host": float(np.median(samples["host"])),
           "plane_bytes": plane_bytes, "us_planes_at_hbm_rate": 1e6 * plane_bytes / HBM_BYTES_PER_S}
    res["ratio_device_over_host"] = res["images_per_s_device"] / res["images_per_s_host"]
    c.close()
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
