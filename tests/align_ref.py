"""numpy restatement of the azimuth registration (include/radarays_mi355.h, rr_align_images_device): the circular
cross-correlation of two uint8 polar images over all azimuth shifts as an int64 Gram matrix product with its wrapped diagonals
summed, and the record the library forms from it in exact Python integers."""
import math

import numpy as np


def window(x, cell_begin=0, cell_end=None):
    x = np.asarray(x)
    return x[cell_begin:x.shape[0] if cell_end is None else cell_end]


def xcorr_roll(x, r, cell_begin=0, cell_end=None):
    """the literal definition: xcorr[s] = sum(np.roll(x, s, axis=1) * r) over the cell window, int64 [n_angles]"""
    x, r = window(x, cell_begin, cell_end).astype(np.int64), window(r, cell_begin, cell_end).astype(np.int64)
    return np.array([int((np.roll(x, s, axis=1) * r).sum()) for s in range(x.shape[1])], np.int64)


def xcorr(x, r, cell_begin=0, cell_end=None):
    """the same curve from G = x^T r (int64 [n_angles][n_angles]): xcorr[s] = sum_a G[a][(a + s) mod n_angles].  The product
    runs through BLAS in f64, where it is exact -- every partial sum is an integer of at most 255^2 x cells, far below 2^53 --
    and is converted to int64 before the diagonals are summed (numpy's own int64 matmul gives the same matrix, seconds slower)"""
    x, r = window(x, cell_begin, cell_end), window(r, cell_begin, cell_end)
    A = x.shape[1]
    assert 255 * 255 * x.shape[0] < 2 ** 53
    G = (x.T.astype(np.float64) @ r.astype(np.float64)).astype(np.int64)
    a = np.arange(A)
    return G[a[:, None], (a[:, None] + a[None, :]) % A].sum(axis=0)


def psnr_of(sse, n):
    return math.inf if sse == 0 else 10.0 * math.log10(255.0 ** 2 / (sse / n))


def ncc_of(n, xc, sx, sxx, sr, srr):
    num, fx, fr = n * xc - sx * sr, n * sxx - sx * sx, n * srr - sr * sr
    return 0.0 if fx == 0 or fr == 0 else float(num) / math.sqrt(float(fx) * float(fr))


def align(x, r, cell_begin=0, cell_end=None, curve=None):
    """the rr_align_record of image x against reference r as a dict (Python integers; psnr and ncc floats) plus "curve"""
    xw, rw = window(x, cell_begin, cell_end).astype(np.int64), window(r, cell_begin, cell_end).astype(np.int64)
    c = xcorr(x, r, cell_begin, cell_end) if curve is None else np.asarray(curve, np.int64)
    n = int(xw.size)
    sx, sxx, sr, srr = int(xw.sum()), int((xw * xw).sum()), int(rw.sum()), int((rw * rw).sum())
    top = int(c.max())
    shift = int(np.argmax(c))                         # the first (smallest) s that attains the maximum
    sse = sxx + srr - 2 * top
    return {"shift": shift, "n_best": int((c == top).sum()), "xcorr": top, "sse": sse, "psnr": psnr_of(sse, n),
            "ncc": ncc_of(n, top, sx, sxx, sr, srr), "sum_x": sx, "sum_xx": sxx, "sum_r": sr, "sum_rr": srr, "curve": c}
