"""Azimuth registration on the card: 1, 16 and 64 images of 3424 x 400 against one reference image, the
circular cross-correlation over all 400 shifts three ways.

    python tools/probe_align.py [--reps 20] [--rounds 3] [--json out.json]
    python tools/probe_align.py --kernels-only        # the library's calls alone, for rocprofv3 --kernel-trace --stats

1. rr_align_images_device: a host clock around a synchronous call (launches, the copy of the records and the synchronise
   included), curve into a caller's buffer.
2. What a user would write today with torch: fp32 `x.T @ r` per image (batched) and the wrapped diagonal sums by a gather.
   fp32 is NOT exact here (a Gram entry reaches 2.2e8 > 2^24); its largest error against the exact curve is reported.
3. torch.fft: rfft along the azimuth, the product with the conjugate summed over the cells, irfft; fp32, its error reported too.
The three are alternated inside each round; the median over the rounds and the spread are reported.  Every route's curve is
checked against the library's (exact) curve before anything is timed.  The bytes-once bound: every image and the reference read
once, (n + 1) x 1.37 MB, over the HBM rate a plain device copy of 256 MB reaches in the same session."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from radarays_ros_amd import native, params  # noqa: E402

NS = (1, 16, 64)


def dark(rs, shape):
    img = rs.randint(0, 30, shape).astype(np.uint8)
    peaks = rs.rand(*shape) < 0.02
    img[peaks] = rs.randint(80, 256, int(peaks.sum()))
    return img


def gemm_route(x, r, idx):
    """x uint8 [n][C][A], r uint8 [C][A] -> fp32 curve [n][A]: G = x^T r per image, c[s] = sum_a G[a][(a + s) % A]"""
    G = torch.matmul(x.float().transpose(1, 2), r.float())
    return torch.gather(G, 2, idx.expand(G.shape[0], -1, -1)).sum(dim=1)


def fft_route(x, r):
    """c[s] = sum_c sum_a x[c][a] r[c][a + s] = irfft(sum_c conj(X_c) R_c)"""
    X, R = torch.fft.rfft(x.float(), dim=2), torch.fft.rfft(r.float(), dim=1)
    return torch.fft.irfft((torch.conj(X) * R).sum(dim=1), n=x.shape[2], dim=1)


def timed(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()

    cfg = params.kaist_preset()
    n_cells, n_angles = cfg.n_cells, params.N_ANGLES
    npx = n_cells * n_angles
    ctx = native.Context(0)
    ctx.set_config(cfg, n_angles)
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(11)
    ref = dark(rs, (n_cells, n_angles))
    base = np.stack([np.roll(ref, 11, axis=1)] + [dark(rs, (n_cells, n_angles)) for _ in range(3)])
    imgs = torch.from_numpy(base).to(dev)[torch.arange(max(NS)) % len(base)].contiguous()
    d_ref = torch.from_numpy(ref).to(dev)
    curve = torch.zeros((max(NS), n_angles), dtype=torch.int64, device=dev)
    ar = torch.arange(n_angles, device=dev)
    idx = ((ar[:, None] + ar[None, :]) % n_angles)[None]
    out = {"n_cells": n_cells, "n_angles": n_angles, "reps": a.reps, "rounds": a.rounds}

    rec = ctx.align_images_device(imgs.data_ptr(), max(NS), d_ref.data_ptr(), 0, None, curve.data_ptr())
    assert rec["shift"][0] == n_angles - 11 and rec["sse"][0] == 0, rec[0]
    exact = curve.clone()
    if a.kernels_only:
        for n in NS:
            for _ in range(a.reps):
                ctx.align_images_device(imgs.data_ptr(), n, d_ref.data_ptr(), 0, None, curve.data_ptr())
        return emit(out, a)

    # the HBM rate of this session: a device-to-device copy of 256 MB reads and writes it once
    src = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    us = timed(lambda: dst.copy_(src), 20)
    out["hbm_copy_bytes_per_s"] = 2 * src.numel() / (us * 1e-6)
    print("device copy of 256 MB: %.1f us, %.2f TB/s read + write" % (us, out["hbm_copy_bytes_per_s"] / 1e12), flush=True)
    del src, dst

    for n in NS:
        x = imgs[:n]
        routes = {"align": lambda: ctx.align_images_device(x.data_ptr(), n, d_ref.data_ptr(), 0, None, curve.data_ptr()),
                  "torch_gemm_fp32": lambda: gemm_route(x, d_ref, idx),
                  "torch_fft": lambda: fft_route(x, d_ref)}
        err = {"torch_gemm_fp32": float((gemm_route(x, d_ref, idx).double() - exact[:n].double()).abs().max()),
               "torch_fft": float((fft_route(x, d_ref).double() - exact[:n].double()).abs().max())}
        times = {k: [] for k in routes}
        for fn in routes.values():                   # warm-up of every shape the timed window uses
            for _ in range(3):
                fn()
        for _ in range(a.rounds):
            for k, fn in routes.items():
                times[k].append(timed(fn, a.reps))
        floor = (n + 1) * npx / out["hbm_copy_bytes_per_s"] * 1e6
        out["n%d" % n] = {"us": {k: [round(t, 1) for t in v] for k, v in times.items()}, "median_us": {k: round(float(np.median(v)), 1) for k, v in times.items()},
                         "max_abs_error": err, "bytes_once_floor_us": round(floor, 2)}
        print("n = %2d: %s; bytes-once floor %.2f us; max |error| of the fp32 routes %s (xcorr peaks at %.3g)" % (
            n, ", ".join("%s %.1f us (%s)" % (k, np.median(v), " ".join("%.0f" % t for t in v)) for k, v in times.items()), floor,
            err, float(exact[:n].max())), flush=True)
    return emit(out, a)


def emit(out, a):
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
