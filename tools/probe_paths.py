"""Wave paths on the card: the routes of a frame's ghosts on the bench scene, and what rr_simulate_batch_paths_device
costs beside rr_simulate_batch_device.

    python tools/probe_paths.py [--workload target] [--azimuth 100] [--reps 20] [--rounds 3] [--json out.json]

For the first pose of the workload's trajectory (bench.py's: config 2 = 100k triangles, 1 pass; target = 10M triangles, 4 passes;
400 azimuths x 200 beam samples, ambient noise 2, record_multi_path on so that later passes echo twice):
1. per pass the waves cast and the share that hit, over all azimuths (RadarHIP-level call: rr_simulate_paths, map frame);
2. for the three strongest ghost echoes (pass > 0) of --azimuth, the route: per wave of the chain its face, object and segment length,
   from the beam to the echo (radar.path_to_echo), with the echo's range bin and strength from the provenance stream of the same pose;
3. images/s of the plain batch and of the paths call (records of every wave into device rows) at 1 and 8 frames per call: a host clock
   around --reps calls and one synchronise, routes alternated inside each round, median; and k_wave_gather alone from the context's
   kernel timer ("waves") in timing mode, microseconds per launch.
Before anything is timed the paths call's images are compared with the plain batch's.  One JSON line at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from radarays_ros_amd import native, params, radar, scenes  # noqa: E402
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


def routes_of(c, pose, az):
    """the wave lists of the frame, the pass table, and the three strongest ghosts of azimuth az with their routes"""
    u8, wav, cnt, pc = c.simulate_paths(pose, map_frame=True)
    _, _, _, ech, ecnt = c.simulate_provenance(pose, want_labels=False, want_faces=False)
    passes = []
    for p in range(c.cfg.n_reflections):
        m = (np.arange(wav.shape[1])[None, :] < cnt[:, None]) & (radar.unpack_wave_info(wav["info"])[1] == p)
        cast = int(m.sum())
        passes.append({"pass": p, "waves": cast, "hit_share": float((wav["range"][m] >= 0).mean()) if cast else None})
        print("pass %d: %9d waves cast, %5.1f %% hit" % (p, cast, 100.0 * (passes[-1]["hit_share"] or 0.0)))
    w, e = wav[az, :cnt[az]], ech[az, :ecnt[az]]
    ghost = np.flatnonzero(native.unpack_info(e["info"])[1] > 0)
    ghosts = []
    for k in ghost[np.argsort(-e["strength"][ghost], kind="stable")[:3]]:
        chain, pts = radar.path_to_echo(w, k)
        obj = radar.unpack_wave_info(w["info"][chain])[0]
        seg = np.linalg.norm(np.diff(pts.astype(np.float64), axis=0), axis=1)
        ghosts.append({"echo": int(k), "cell": int(e["cell"][k]), "strength": float(e["strength"][k]), "kind": int(native.unpack_info(e["info"][k])[2]),
                       "waves": chain.tolist(), "faces": w["face"][chain].tolist(), "objects": obj.tolist(), "segments_m": seg.tolist()})
        print("azimuth %d, echo %d (bin %d, strength %.4g, %s): %s" % (
            az, k, e["cell"][k], e["strength"][k], "multipath" if ghosts[-1]["kind"] else "path",
            " -> ".join("face %d / object %d after %.2f m" % (f, o, s) for f, o, s in zip(ghosts[-1]["faces"], ghosts[-1]["objects"], seg))))
    return {"passes": passes, "waves_per_azimuth_mean": float(cnt.mean()), "waves_per_azimuth_max": int(cnt.max()), "azimuth": az, "ghosts": ghosts}, int(cnt.max())


def probe(name, az, reps, rounds):
    scene_id, n_passes, n_beam = WORKLOADS[name]
    s = scenes.config_scene(scene_id)
    cfg = params.kaist_preset(n_reflections=n_passes, ambient_noise=2, record_multi_path=True)
    c = native.Context(0)
    c.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    c.set_materials(materials_for(s), s["object_materials"], 0)
    c.set_config(cfg)
    c.set_beam_samples(golden_beams(n_beam))
    c.set_noise_offsets((np.random.RandomState(7).uniform(0, 1, 400) * 1000).astype(np.float32))
    traj = np.stack(scenes.trajectory(16, s["name"]))
    out, longest = routes_of(c, traj[0], az)
    cap = n_beam * (2 ** (n_passes - 1))
    stride = sum(min(n_beam << p, cap) for p in range(n_passes))          # no list can get longer
    out["wave_stride"] = stride
    for frames in (1, 8):
        batch = lambda k: traj[(np.arange(frames) + k * frames) % 16]   # noqa: E731
        img = torch.zeros((frames, cfg.n_cells, 400), dtype=torch.uint8, device=DEV)
        img2 = torch.zeros_like(img)
        wav = torch.zeros((frames * 400 * stride * 64,), dtype=torch.uint8, device=DEV)
        cnt = torch.zeros((frames, 400), dtype=torch.int32, device=DEV)
        fns = {"plain": lambda k: c.simulate_batch_device(batch(k), img.data_ptr()),
               "paths": lambda k: c.simulate_batch_paths_device(batch(k), img2.data_ptr(), wav.data_ptr(), stride, cnt.data_ptr())}
        fns["plain"](0); fns["paths"](0)
        c.synchronize()
        out["images_equal_plain_%d" % frames] = bool(torch.equal(img, img2))
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
            fns["paths"](k)
        c.synchronize()
        for kern in ("waves", "shade"):
            ms, n = c.kernel_time(kern, True)
            out["us_per_launch_%s_%d" % (kern, frames)] = 1e3 * ms / n if n else None
        c.set_timing_mode(0)
        del wav
    c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="target", choices=sorted(WORKLOADS))
    ap.add_argument("--azimuth", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = {"tool": "probe_paths", "device": torch.cuda.get_device_name(0), a.workload: probe(a.workload, a.azimuth, a.reps, a.rounds)}
    line = json.dumps(res)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
