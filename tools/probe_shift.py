"""Translation registration on the card: 1, 16 and 64 images of 1024 x 1024 against one reference image, the
2-D cross-correlation over the 65 x 65 shifts of max_shift = 32 three ways.

    python tools/probe_shift.py [--reps 10] [--rounds 3] [--torch-reps 2] [--json out.json]
    python tools/probe_shift.py --kernels-only        # the library's calls alone, for rocprofv3 --kernel-trace --stats

1. rr_shift_images_device: a host clock around a synchronous call (launches, the copy of the records and the synchronise
   included), both surfaces into a caller's buffers.
2. What a user would write today with torch: fp32 conv2d (which is a correlation) of the reference with every image's template
   window as a 960 x 960 filter.  fp32 is NOT exact here (xcorr reaches 1e10 > 2^24); its largest error against the exact
   surface is reported.  A route whose first call takes longer than --give-up seconds is timed on that one call only.
3. torch.fft: rfft2 of the reference and of the template (zero outside T), the product with the conjugate, irfft2, the 65 x 65
   corner; fp32, its error reported too.
The routes are alternated inside each round; the median over the rounds is reported.  Every route's surface is compared with
the library's (exact) surface before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from radarays_ros_amd import native  # noqa: E402

NS = (1, 16, 64)
H = W = 1024
S = 32
D = 2 * S + 1


def dark(rs, shape):
    img = rs.randint(0, 30, shape).astype(np.uint8)
    peaks = rs.rand(*shape) < 0.02
    img[peaks] = rs.randint(80, 256, int(peaks.sum()))
    return img


def conv_route(x, r):
    """x uint8 [n][H][W], r uint8 [H][W] -> fp32 surface [n][D][D]"""
    return torch.nn.functional.conv2d(r.float()[None, None], x[:, None, S:H - S, S:W - S].float())[0]


def fft_route(x, r):
    t = torch.zeros(x.shape, dtype=torch.float32, device=x.device)
    t[:, S:H - S, S:W - S] = x[:, S:H - S, S:W - S].float()
    c = torch.fft.irfft2(torch.conj(torch.fft.rfft2(t)) * torch.fft.rfft2(r.float())[None], s=(H, W))
    d = torch.arange(-S, S + 1, device=x.device)
    return c[:, d % H][:, :, d % W]


def timed(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--give-up", type=float, default=5.0)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()

    ctx = native.Context(0)
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(12)
    ref = dark(rs, (H, W))
    base = np.stack([np.roll(ref, (-5, 11), axis=(0, 1))] + [dark(rs, (H, W)) for _ in range(3)])
    imgs = torch.from_numpy(base).to(dev)[torch.arange(max(NS)) % len(base)].contiguous()
    d_ref = torch.from_numpy(ref).to(dev)
    xc = torch.zeros((max(NS), D, D), dtype=torch.int64, device=dev)
    sse = torch.zeros((max(NS), D, D), dtype=torch.int64, device=dev)
    out = {"height": H, "width": W, "max_shift": S, "reps": a.reps, "torch_reps": a.torch_reps, "rounds": a.rounds}

    def lib(n):
        return ctx.shift_images_device(imgs.data_ptr(), n, d_ref.data_ptr(), H, W, S, xc.data_ptr(), sse.data_ptr())
    rec = lib(max(NS))
    assert (rec["dy"][0], rec["dx"][0]) == (5, -11) and rec["sse"][0] == 0, rec[0]
    exact = xc.clone()
    if a.kernels_only:
        for n in NS:
            for _ in range(a.reps):
                lib(n)
        return emit(out, a)

    for n in NS:
        x = imgs[:n]
        routes = {"shift": (lambda: lib(n), a.reps), "torch_conv2d_fp32": (lambda: conv_route(x, d_ref), a.torch_reps),
                  "torch_fft": (lambda: fft_route(x, d_ref), a.torch_reps)}
        err, times, once = {}, {k: [] for k in routes}, {}
        for k, (fn, _) in routes.items():                # the first call: checked against the exact surface, and how long it takes
            torch.cuda.synchronize()
            t = time.perf_counter()
            got = fn()
            torch.cuda.synchronize()
            once[k] = time.perf_counter() - t
            if k != "shift":
                err[k] = float((got.double() - exact[:n].double()).abs().max())
        for _ in range(a.rounds):
            for k, (fn, reps) in routes.items():
                if once[k] > a.give_up:
                    continue                             # too slow to repeat: the first call stands for it
                times[k].append(timed(fn, reps))
        med = {k: round(float(np.median(v)), 1) if v else round(once[k] * 1e6, 1) for k, v in times.items()}
        out["n%d" % n] = {"us": {k: [round(t, 1) for t in v] for k, v in times.items()}, "median_us": med,
                         "first_call_s": {k: round(v, 4) for k, v in once.items()}, "max_abs_error": err,
                         "ratio_to_shift": {k: round(med[k] / med["shift"], 2) for k in med if k != "shift"}}
        print("n = %2d: %s; max |error| of the fp32 routes %s (xcorr peaks at %.3g)" % (
            n, ", ".join("%s %.1f us" % (k, v) for k, v in med.items()), err, float(exact[:n].max())), flush=True)
    return emit(out, a)


def emit(out, a):
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
