"""Real-to-sim image metrics on the card: 16 images of 3424 x 400 against one reference image.

    python tools/probe_metrics.py [--reps 20] [--json out.json]
    python tools/probe_metrics.py --kernels-only --set dark|sim      # the metric calls alone, for rocprofv3 --kernel-trace --stats
    RR_METRICS_HIST=1 python tools/probe_metrics.py --kernels-only ...   # the joint histogram with global atomics instead

Two image sets: `dark` (synthetic: noise below 30 with 2 % strong peaks, the reference another draw of the same) and `sim`
(16 poses simulated on config 2, the reference a 17th pose).
1. Call time of rr_compare_images_device per mask (PSNR / SSIM / INFO / all): a host clock around a synchronous call, so
   it includes the launches, the copy of the records and the synchronise.  Kernel times come from a kernel trace of
   --kernels-only (k_score, k_joint_hist, k_ssim, k_metrics_finish), not from here.
2. The yardsticks: what simulating those 16 images on config 2 takes (rr_simulate_batch_device, synchronised), and each
   kernel's HBM byte floor at 8 TB/s, from the shapes.
3. Objective evaluations per second of the parameter batch (tools/probe_sets.py is the model: K sets per call, scores
   only): rr_simulate_param_sets (PSNR) against rr_simulate_param_sets_metrics with SSIM | INFO and with all three,
   alternated in one session."""
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

F = 16
MASKS = {"psnr": native.METRIC_PSNR, "ssim": native.METRIC_SSIM, "info": native.METRIC_INFO, "all": native.METRIC_ALL}
HBM_BYTES_PER_S = 8.0e12


def dark_set(n_cells, n_angles):
    rs = np.random.RandomState(11)

    def one():
        img = rs.randint(0, 30, (n_cells, n_angles)).astype(np.uint8)
        peaks = rs.rand(n_cells, n_angles) < 0.02
        img[peaks] = rs.randint(80, 256, int(peaks.sum()))
        return img
    return np.stack([one() for _ in range(F)]), one()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sets", type=int, default=8, help="parameter sets per call")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--set", choices=["dark", "sim", "both"], default="both")
    ap.add_argument("--win", type=int, default=7)
    ap.add_argument("--json")
    a = ap.parse_args()

    t0 = time.time()
    scene = scenes.config_scene(2)
    cfg = params.kaist_preset(n_reflections=1, n_samples=200, ambient_noise=2)
    mats = materials_for(scene)
    ctx = native.Context(0)
    ctx.set_mesh(scene["verts"], scene["faces"], scene["face_object_id"])
    ctx.set_materials(mats, scene["object_materials"], 0)
    ctx.set_config(cfg, params.N_ANGLES)
    ctx.set_beam_samples(golden_beams(200))
    ctx.set_noise_offsets((np.random.RandomState(7).uniform(0, 1, 17 * params.N_ANGLES) * 1000.0).astype(np.float32))
    poses = scenes.trajectory(F + 1, scene["name"])
    n_cells, n_angles = cfg.n_cells, params.N_ANGLES
    npx = n_cells * n_angles
    print("scene %s, %d triangles, set up in %.1f s; histogram shape %s" % (
        scene["name"], len(scene["faces"]), time.time() - t0, os.environ.get("RR_METRICS_HIST", "0")), flush=True)

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    out = {"frames": F, "n_cells": n_cells, "n_angles": n_angles, "win_size": a.win, "hist_shape": int(os.environ.get("RR_METRICS_HIST", "0"))}
    sim = torch.empty((F + 1, n_cells, n_angles), dtype=torch.uint8, device=dev)
    ctx.simulate_batch_device(poses, sim.data_ptr(), s)
    ctx.synchronize(s)
    d_imgs, d_ref = dark_set(n_cells, n_angles)
    dark = torch.from_numpy(np.concatenate([d_imgs, d_ref[None]])).to(dev)
    torch.cuda.synchronize()
    sets = {"dark": dark, "sim": sim}
    if a.set != "both":
        sets = {a.set: sets[a.set]}

    for name, buf in sets.items():
        imgs, ref = buf.data_ptr(), buf[F].data_ptr()
        for mask_name, mask in MASKS.items():
            if a.kernels_only and mask_name == "all":
                continue
            ctx.compare_images_device(imgs, F, ref, mask, a.win, None, s)
            t = time.perf_counter()
            for _ in range(a.reps):
                rec = ctx.compare_images_device(imgs, F, ref, mask, a.win, None, s)
            us = (time.perf_counter() - t) / a.reps * 1e6
            out["%s_%s_call_us" % (name, mask_name)] = round(us, 1)
            print("%-5s %-5s %9.1f us per call of %d images" % (name, mask_name, us, F), flush=True)
        rec = ctx.compare_images_device(imgs, F, ref, native.METRIC_ALL, a.win, None, s)
        out[name + "_means"] = {k: float(np.mean(rec[k][np.isfinite(rec[k])])) for k in ("psnr", "ssim", "mi", "nmi", "voi")}
        print("%-5s mean psnr %.2f dB, ssim %.4f, mi %.4f nats, nmi %.4f, voi %.4f" % ((name,) + tuple(out[name + "_means"].values())), flush=True)
    # floors from the shapes: every image and the reference read once; the histograms zeroed, written and read once
    tiles = ((n_cells - a.win + 1 + 31) // 32) * ((n_angles - a.win + 1 + 63) // 64)
    floors = {"k_score": (F + 1) * npx, "k_joint_hist": (F + 1) * npx + 2 * F * 65536 * 4, "k_ssim": (F + 1) * npx + F * tiles * 8,
              "k_metrics_finish": F * 65536 * 4 + F * tiles * 8}
    out["hbm_floor_us"] = {k: round(v / HBM_BYTES_PER_S * 1e6, 2) for k, v in floors.items()}
    print("HBM byte floors at 8 TB/s (us):", out["hbm_floor_us"], flush=True)
    if a.kernels_only:
        return emit(out, a)

    # the yardstick: simulating those 16 images
    for _ in range(3):
        ctx.simulate_batch_device(poses[:F], sim.data_ptr(), s)
    ctx.synchronize(s)
    t = time.perf_counter()
    for _ in range(a.reps):
        ctx.simulate_batch_device(poses[:F], sim.data_ptr(), s)
    ctx.synchronize(s)
    out["simulate_16_images_us"] = round((time.perf_counter() - t) / a.reps * 1e6, 1)
    print("simulate %d images on config 2: %.1f us per batch" % (F, out["simulate_16_images_us"]), flush=True)

    # the parameter batch, scores only
    K = a.sets
    base = np.asarray([m.astuple() for m in mats], np.float32)
    rs = np.random.RandomState(1)
    tables = np.repeat(base[None], K, axis=0)
    tables[:, 1:, 2] = rs.uniform(0, 1, (K, len(mats) - 1))
    psets = [{"materials": tables[k]} for k in range(K)]
    real = sim[F].cpu().numpy()
    pose = poses[0]
    forms = {"psnr_only": lambda: ctx.simulate_param_sets(pose, psets, len(mats), ref_u8=real, want_images=False),
             "metrics_psnr": lambda: ctx.simulate_param_sets(pose, psets, len(mats), ref_u8=real, want_images=False, metrics=native.METRIC_PSNR),
             "metrics_ssim_info": lambda: ctx.simulate_param_sets(pose, psets, len(mats), ref_u8=real, want_images=False,
                                                                  metrics=native.METRIC_SSIM | native.METRIC_INFO, win_size=a.win),
             "metrics_all": lambda: ctx.simulate_param_sets(pose, psets, len(mats), ref_u8=real, want_images=False, metrics=native.METRIC_ALL, win_size=a.win)}
    rates = {k: [] for k in forms}
    for fn in forms.values():
        for _ in range(3):
            fn()
    for _ in range(3):                       # alternated, three rounds: the spread is reported
        for k, fn in forms.items():
            n = 3 * a.reps
            t = time.perf_counter()
            for _ in range(n):
                fn()
            rates[k].append(n * K / (time.perf_counter() - t))
    for k, v in rates.items():
        out["evals_per_s_" + k] = [round(x, 1) for x in v]
        print("%-18s %s evaluations/s (K = %d per call)" % (k, ", ".join("%.0f" % x for x in v), K), flush=True)
    med = {k: float(np.median(v)) for k, v in rates.items()}
    out["ratio_ssim_info_to_psnr_only"] = round(med["metrics_ssim_info"] / med["psnr_only"], 4)
    out["ratio_all_to_psnr_only"] = round(med["metrics_all"] / med["psnr_only"], 4)
    print("SSIM | INFO / PSNR-only: %.4f; all / PSNR-only: %.4f" % (out["ratio_ssim_info_to_psnr_only"], out["ratio_all_to_psnr_only"]))
    return emit(out, a)


def emit(out, a):
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
