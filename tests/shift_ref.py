"""numpy restatement of the translation registration (include/radarays_mi355.h, rr_shift_images_device): the 2-D
cross-correlation of two uint8 images over the shifts -S..S as a family of banded Gram products, one per dy, with their
diagonals summed -- beside the literal slice form -- and the record the library forms from it in exact Python integers.
Surfaces are indexed [dy + S][dx + S]."""
import math

import numpy as np

import align_ref as A

U64_MAX = 2 ** 64 - 1


def xcorr_literal(x, r, S):
    """the literal definition: xcorr[dy][dx] = (x[T] * r[T + (dy, dx)]).sum(), int64 [2S+1][2S+1]"""
    x, r = np.asarray(x).astype(np.int64), np.asarray(r).astype(np.int64)
    H, W = x.shape
    xt = x[S:H - S, S:W - S]
    out = np.zeros((2 * S + 1, 2 * S + 1), np.int64)
    for g in range(2 * S + 1):
        for f in range(2 * S + 1):
            out[g, f] = int((xt * r[g:g + H - 2 * S, f:f + W - 2 * S]).sum())
    return out


def xcorr(x, r, S):
    """the same surface from G_dy = x[T]^T r[rows of T moved by dy] (int64 [W-2S][W]): element (a, b) belongs to dx = b - a,
    so xcorr[dy][dx] = sum_a G_dy[a][a + dx].  The products run through BLAS in f64, where they are exact -- every partial sum
    is an integer of at most 255^2 x 8192 rows < 2^53 -- and are converted to int64 before the diagonals are summed"""
    x, r = np.asarray(x), np.asarray(r)
    H, W = x.shape
    assert 255 * 255 * H < 2 ** 53
    xt = x[S:H - S, S:W - S].astype(np.float64).T.copy()
    a = np.arange(W - 2 * S)[:, None]                   # image column a + S meets reference column a + S + dx = a + f
    f = np.arange(2 * S + 1)[None, :]
    out = np.zeros((2 * S + 1, 2 * S + 1), np.int64)
    for g in range(2 * S + 1):
        G = (xt @ r[g:g + H - 2 * S].astype(np.float64)).astype(np.int64)
        out[g] = G[a, a + f].sum(axis=0)
    return out


def box_sums(r, S):
    """(Sr, Srr): the sums of r and r^2 over T moved by every shift, exact int64 [2S+1][2S+1], from integral images"""
    r = np.asarray(r).astype(np.int64)
    H, W = r.shape
    h, w = H - 2 * S, W - 2 * S
    out = []
    for v in (r, r * r):
        I = np.zeros((H + 1, W + 1), np.int64)
        I[1:, 1:] = v.cumsum(axis=0).cumsum(axis=1)
        out.append(I[h:h + 2 * S + 1, w:w + 2 * S + 1] - I[0:2 * S + 1, w:w + 2 * S + 1] - I[h:h + 2 * S + 1, 0:2 * S + 1] + I[0:2 * S + 1, 0:2 * S + 1])
    return out[0], out[1]


def sub_of(before, at_best, after):
    """the sub-pixel offset along one axis from the exact SSE before, at and after the best shift"""
    if before == U64_MAX or after == U64_MAX:
        return 0.0
    num, den = before - after, before - 2 * at_best + after
    return 0.0 if den <= 0 else 0.5 * float(num) / float(den)


def shift(x, r, S, surface=None, box=None):
    """the rr_shift_record of image x against reference r as a dict (Python integers; psnr, ncc, sub_* floats) plus the
    surfaces "xcorr_surface" (int64) and "sse_surface" (uint64)"""
    x, r = np.asarray(x), np.asarray(r)
    H, W = x.shape
    D = 2 * S + 1
    n = (H - 2 * S) * (W - 2 * S)
    xc = xcorr(x, r, S) if surface is None else np.asarray(surface, np.int64)
    Sr, Srr = box_sums(r, S) if box is None else box
    xt = x[S:H - S, S:W - S].astype(np.int64)
    sx, sxx = int(xt.sum()), int((xt * xt).sum())
    sse = sxx + Srr - 2 * xc                             # int64: every entry is >= 0 and below 2^40
    assert sse.min() >= 0
    low = int(sse.min())
    d = int(np.argmin(sse))                              # the first (smallest) index that attains the minimum
    g, f = divmod(d, D)
    nb = [int(sse[g - 1, f]) if g > 0 else U64_MAX, int(sse[g + 1, f]) if g < D - 1 else U64_MAX,
          int(sse[g, f - 1]) if f > 0 else U64_MAX, int(sse[g, f + 1]) if f < D - 1 else U64_MAX]
    top, sr, srr = int(xc[g, f]), int(Sr[g, f]), int(Srr[g, f])
    return {"dy": g - S, "dx": f - S, "n_best": int((sse == low).sum()), "xcorr": top, "sse": low, "psnr": A.psnr_of(low, n),
            "ncc": A.ncc_of(n, top, sx, sxx, sr, srr), "sub_dy": sub_of(nb[0], low, nb[1]), "sub_dx": sub_of(nb[2], low, nb[3]),
            "sse_nb": nb, "sum_x": sx, "sum_xx": sxx, "sum_r": sr, "sum_rr": srr,
            "xcorr_surface": xc, "sse_surface": sse.astype(np.uint64)}
