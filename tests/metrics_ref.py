"""numpy / scipy restatement of the image metrics of include/radarays_mi355.h (rr_compare_images_device): SSIM written the
way skimage.metrics.structural_similarity writes it for uint8 images with its defaults, the joint histogram, and the
entropies.  The GPU tests compare the library with this file; tests/test_metrics_host.py pins this file to sklearn and to an
integer-window-sum form of SSIM; tests/test_metrics_edges_host.py pins both to ssim_map, the S of every window position."""
import numpy as np
from scipy.ndimage import uniform_filter


def ssim(x, y, win_size=7):
    """skimage.metrics.structural_similarity(x, y) for uint8 images: uniform window, K1 0.01, K2 0.03, data_range 255,
    sample covariance, the mean over the pixels whose window lies inside the image (crop by (win_size - 1) / 2)"""
    x = np.asarray(x).astype(np.float64)
    y = np.asarray(y).astype(np.float64)
    K1, K2, R = 0.01, 0.03, 255
    NP = win_size ** 2
    cov_norm = NP / (NP - 1)
    f = dict(size=win_size)
    ux, uy = uniform_filter(x, **f), uniform_filter(y, **f)
    uxx, uyy, uxy = uniform_filter(x * x, **f), uniform_filter(y * y, **f), uniform_filter(x * y, **f)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    C1, C2 = (K1 * R) ** 2, (K2 * R) ** 2
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux ** 2 + uy ** 2 + C1, vx + vy + C2
    S = (A1 * A2) / (B1 * B2)
    pad = (win_size - 1) // 2
    return float(S[pad:S.shape[0] - pad, pad:S.shape[1] - pad].mean(dtype=np.float64))


def ssim_integer(x, y, win_size=7):
    """the same number from exact integer window sums (summed-area tables), S in f64: the form the kernel computes"""
    x = np.asarray(x).astype(np.int64)
    y = np.asarray(y).astype(np.int64)
    w = win_size

    def wsum(a):
        s = np.zeros((a.shape[0] + 1, a.shape[1] + 1), np.int64)
        s[1:, 1:] = a.cumsum(0).cumsum(1)
        return (s[w:, w:] - s[:-w, w:] - s[w:, :-w] + s[:-w, :-w]).astype(np.float64)
    NP = float(w * w)
    cov_norm = NP / (NP - 1)
    ux, uy, uxx, uyy, uxy = wsum(x) / NP, wsum(y) / NP, wsum(x * x) / NP, wsum(y * y) / NP, wsum(x * y) / NP
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return float(S.mean(dtype=np.float64))


def ssim_map(x, y, win_size=7):
    """S of every window position, [n_rows - w + 1][n_cols - w + 1] in the window's corner coordinates, from window sums taken
    by brute force (every window's w x w pixels added up in int64; no summed-area table, no filter) and the f64 expression of
    ssim_integer.  Its mean is the SSIM; a third route to it, and the only one that says where a position's share lies"""
    from numpy.lib.stride_tricks import sliding_window_view
    x = np.asarray(x).astype(np.int64)
    y = np.asarray(y).astype(np.int64)
    w = win_size

    def wsum(a):
        return sliding_window_view(a, (w, w)).sum(axis=(2, 3)).astype(np.float64)
    NP = float(w * w)
    cov_norm = NP / (NP - 1)
    ux, uy, uxx, uyy, uxy = wsum(x) / NP, wsum(y) / NP, wsum(x * x) / NP, wsum(y * y) / NP, wsum(x * y) / NP
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def joint_histogram(x, y):
    """H[a][b] = pixels with x == a and y == b, uint32 [256][256]"""
    H = np.zeros((256, 256), np.uint32)
    np.add.at(H, (np.asarray(x).ravel().astype(np.intp), np.asarray(y).ravel().astype(np.intp)), 1)
    return H


def entropy(counts):
    """ln N - (1/N) sum c ln c in nats over the non-empty bins, summed as (1/N) sum c (ln N - ln c): 0 exactly when one bin
    holds everything"""
    c = np.asarray(counts, np.float64).ravel()
    n = c.sum()
    c = c[c > 0]
    return float(np.sum(c * (np.log(n) - np.log(c))) / n)


def info(H):
    H = np.asarray(H, np.float64)
    hx, hy, hxy = entropy(H.sum(1)), entropy(H.sum(0)), entropy(H)
    return {"hx": hx, "hy": hy, "hxy": hxy, "mi": hx + hy - hxy, "nmi": 1.0 if hxy == 0.0 else (hx + hy) / hxy,
            "voi": 2.0 * hxy - hx - hy}


def psnr(x, y):
    """skimage.metrics.peak_signal_noise_ratio for uint8: (sse, 10 log10(255^2 / mse)), +inf for equal images"""
    d = np.asarray(x).astype(np.int64) - np.asarray(y).astype(np.int64)
    sse = int((d * d).sum())
    return sse, (np.inf if sse == 0 else 10.0 * np.log10(255.0 ** 2 / (sse / d.size)))
