"""Doppler on the card: by how many bins a moving vehicle is drawn away from its mesh, and what
rr_simulate_batch_doppler_device costs beside rr_simulate_batch_paths_device.

    python tools/probe_doppler.py [--workload target] [--speed 15] [--gain 0.05] [--reps 20] [--rounds 3] [--json out.json]

1. A room (scenes.box12, object 0) with one vehicle in it (a 4 x 1.8 x 1.5 m box, object 1) that drives towards the sensor at --speed
   m/s; the sensor stands still.  One frame with gain 0 and one with --gain: per first-pass echo of the vehicle the shift in bins (the
   cells of the two calls, echo by echo), its range rate, and the share of the image's pixels that changed.
2. The cost at the workload's shape (bench.py's: config 2 = 100k triangles, 1 pass; target = 10M triangles, 4 passes; 400 azimuths x
   200 beam samples, ambient noise 2, record_multi_path on): images/s of the plain batch, of the paths call (records of every wave)
   and of the Doppler call (rates and cells of every echo, velocity image) at 1 and 8 frames per call -- a host clock around --reps
   calls and one synchronise, routes alternated inside each round, median -- and the Doppler kernels alone from the context's kernel
   timer ("rates", "shift", "winner", and "column", which a Doppler chain launches twice), microseconds per launch.
One JSON line at the end."""
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


def vehicle(speed, gain):
    room = scenes.box12()
    v, f = scenes._box_tris(np.float32([3.0, -0.9, -0.9]), np.float32([7.0, 0.9, 0.6]), vbase=len(room["verts"]))
    s = {"verts": np.concatenate([room["verts"], v]).astype(np.float32), "faces": np.concatenate([room["faces"], f]).astype(np.uint32),
         "face_object_id": np.concatenate([room["face_object_id"], np.full(len(f), 1, np.uint32)]).astype(np.uint32), "object_materials": [1, 1]}
    cfg = params.kaist_preset(n_reflections=2, ambient_noise=0, record_multi_path=True)
    c = native.Context(0)
    c.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    c.set_materials(materials_for(s), s["object_materials"], 0)
    c.set_config(cfg)
    c.set_beam_samples(golden_beams(32))
    c.set_object_twists([[0, 0, 0, 0, 0, 0], [-speed, 0, 0, 0, 0, 0]])          # towards the sensor at the origin
    pose = scenes.yaw_pose(0.0, 0.0, 0.0, 0.0)
    _, _, _, ech, ecnt = c.simulate_provenance(pose, want_labels=False, want_faces=False)
    still, _, _, cel0, cnt, _ = c.simulate_doppler(pose, None, 0.0)
    moved, _, vr, cel1, _, vimg = c.simulate_doppler(pose, None, gain)
    obj, pas, _ = native.unpack_info(ech["info"])
    m = (np.arange(ech.shape[1])[None, :] < ecnt[:, None]) & (obj == 1) & (pas == 0)
    shift = (cel1[m].astype(np.int64) - cel0[m])[cel1[m] >= 0]
    out = {"speed_m_s": speed, "gain_s": gain, "resolution_m": cfg.resolution, "vehicle_first_pass_echoes": int(m.sum()),
           "expected_bins": -speed * gain / cfg.resolution, "shift_bins_median": float(np.median(shift)) if len(shift) else None,
           "shift_bins_min": int(shift.min()) if len(shift) else None, "shift_bins_max": int(shift.max()) if len(shift) else None,
           "range_rate_min": float(vr[m].min()) if m.any() else None, "range_rate_max": float(vr[m].max()) if m.any() else None,
           "pixels_changed_share": float((still != moved).mean()), "velocity_image_pixels": int((~np.isnan(vimg)).sum())}
    print("vehicle at %.1f m/s, gain %.3f s, %.4f m bins: %d first-pass echoes move by %s bins (median %s; closed form %.1f), v_r %.2f .. %.2f m/s; %.2f %% of the pixels change"
          % (speed, gain, cfg.resolution, out["vehicle_first_pass_echoes"], (out["shift_bins_min"], out["shift_bins_max"]), out["shift_bins_median"],
             out["expected_bins"], out["range_rate_min"] or 0.0, out["range_rate_max"] or 0.0, 100.0 * out["pixels_changed_share"]))
    c.close()
    return out


def cost(name, reps, rounds):
    scene_id, n_passes, n_beam = WORKLOADS[name]
    s = scenes.config_scene(scene_id)
    cfg = params.kaist_preset(n_reflections=n_passes, ambient_noise=2, record_multi_path=True)
    c = native.Context(0)
    c.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    c.set_materials(materials_for(s), s["object_materials"], 0)
    c.set_config(cfg)
    c.set_beam_samples(golden_beams(n_beam))
    c.set_noise_offsets((np.random.RandomState(7).uniform(0, 1, 400) * 1000).astype(np.float32))
    n_obj = int(np.max(s["face_object_id"])) + 1 if s["face_object_id"] is not None else 1
    tw = np.zeros((n_obj, 6), np.float32)
    tw[-1] = [3.0, -1.0, 0.0, 0.0, 0.0, 0.1]
    c.set_object_twists(tw)
    traj = np.stack(scenes.trajectory(16, s["name"]))
    cap = n_beam * (2 ** (n_passes - 1))
    stride = sum(min(n_beam << p, cap) for p in range(n_passes))          # no wave list can get longer; an echo list twice that
    out = {"wave_stride": stride, "echo_stride": 2 * stride}
    for frames in (1, 8):
        batch = lambda k: traj[(np.arange(frames) + k * frames) % 16]   # noqa: E731
        vel = np.tile(np.float32([2.0, 0.5, 0.0]), (frames, 1))
        img = torch.zeros((frames, cfg.n_cells, 400), dtype=torch.uint8, device=DEV)
        img2, img3 = torch.zeros_like(img), torch.zeros_like(img)
        wav = torch.zeros((frames * 400 * stride * 64,), dtype=torch.uint8, device=DEV)
        ev = torch.zeros((frames, 400, 2 * stride), dtype=torch.float32, device=DEV)
        ec = torch.zeros((frames, 400, 2 * stride), dtype=torch.int32, device=DEV)
        vi = torch.zeros((frames, cfg.n_cells, 400), dtype=torch.float32, device=DEV)
        cnt = torch.zeros((frames, 400), dtype=torch.int32, device=DEV)
        fns = {"plain": lambda k: c.simulate_batch_device(batch(k), img.data_ptr()),
               "paths": lambda k: c.simulate_batch_paths_device(batch(k), img2.data_ptr(), wav.data_ptr(), stride, cnt.data_ptr()),
               "doppler": lambda k: c.simulate_batch_doppler_device(batch(k), 0.05, img3.data_ptr(), vel, ev.data_ptr(), 2 * stride, cnt.data_ptr(),
                                                                    ec.data_ptr(), vi.data_ptr())}
        for fn in fns.values():          # warm-up: lanes, launch graphs, trace-row history
            for k in range(8):
                fn(k)
        samples = {r: [] for r in fns}
        for _ in range(rounds):
            for r, fn in fns.items():
                samples[r].append(rate(fn, reps, frames))
        for r in fns:
            out["images_per_s_%s_%d" % (r, frames)] = float(np.median(samples[r]))
        c.synchronize()
        c.set_timing_mode(1)
        for k in range(max(4, reps // 4)):
            fns["doppler"](k)
        c.synchronize()
        for kern in ("rates", "shift", "winner", "column", "shade"):
            ms, n = c.kernel_time(kern, True)
            out["us_per_launch_%s_%d" % (kern, frames)] = 1e3 * ms / n if n else None
        c.set_timing_mode(0)
        del wav, ev, ec, vi
    c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="target", choices=sorted(WORKLOADS))
    ap.add_argument("--speed", type=float, default=15.0)
    ap.add_argument("--gain", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = {"tool": "probe_doppler", "device": torch.cuda.get_device_name(0), "vehicle": vehicle(a.speed, a.gain), a.workload: cost(a.workload, a.reps, a.rounds)}
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
