"""numpy restatement of the point-cloud and Cartesian conversions (include/radarays_mi355.h, rr_detect.hip).

The detectors are this build's own definitions (the reference's radar_img_to_pcl is outside its checkout): these functions
state them a second time, independently of the kernels' structure, and the GPU tests compare bit for bit.  float32 where
the header says f32, one rounding per operation, nothing fused."""
import numpy as np

from radarays_ros_amd.native import POINT_DTYPE


def cfar_mask(img, guard, train, min_intensity=0, min_bin=0, scale=1.0):
    """CA-CFAR detections of one image [n_cells][n_angles] (bool, same shape)"""
    z = np.asarray(img).astype(np.int64)
    N = z.shape[0]
    G, T = int(guard), int(train)
    cs = np.concatenate([np.zeros((1,) + z.shape[1:], np.int64), np.cumsum(z, axis=0)])   # cs[j] = z[0] + .. + z[j-1]
    i = np.arange(N)
    llo, lhi = np.maximum(0, i - G - T), i - G - 1
    rlo, rhi = i + G + 1, np.minimum(N - 1, i + G + T)
    nl = np.maximum(0, lhi - llo + 1)
    nr = np.maximum(0, rhi - rlo + 1)
    left = np.where((nl > 0)[:, None], cs[np.clip(lhi + 1, 0, N)] - cs[np.clip(llo, 0, N)], 0)
    right = np.where((nr > 0)[:, None], cs[np.clip(rhi + 1, 0, N)] - cs[np.clip(rlo, 0, N)], 0)
    n = (nl + nr)[:, None]
    S = left + right
    lhs = (z * n).astype(np.float32)
    rhs = np.float32(scale) * S.astype(np.float32)
    return (z >= min_intensity) & (n > 0) & (lhs > rhs) & (i[:, None] >= min_bin)


def kstrongest_mask(img, k, min_intensity=0, min_bin=0):
    """the k largest candidates of every column (value descending, then bin ascending)"""
    z = np.asarray(img).astype(np.int64)
    N = z.shape[0]
    i = np.arange(N)[:, None]
    cand = (z >= min_intensity) & (i >= min_bin)
    key = np.where(cand, (255 - z) * N + i, np.iinfo(np.int64).max)          # the order of the rule, candidates first
    first = np.argsort(key, axis=0, kind="stable")[:k]
    mask = np.zeros(z.shape, bool)
    cols = np.broadcast_to(np.arange(z.shape[1]), first.shape)
    mask[first, cols] = True
    return mask & cand


def detect_frame(img, method=0, guard_cells=2, train_cells=16, k=12, min_intensity=1, min_bin=0, cfar_scale=3.0,
                 scroll=0, theta_min=0.0, theta_inc=-2 * np.pi / 400, resolution=0.0438):
    """-> (points POINT_DTYPE sorted by column then bin, offsets uint32 [n_angles + 1])"""
    img = np.asarray(img)
    N, A = img.shape
    if method == 0:
        mask = cfar_mask(img, guard_cells, train_cells, min_intensity, min_bin, cfar_scale)
    else:
        mask = kstrongest_mask(img, k, min_intensity, min_bin)
    col, b = np.nonzero(mask.T)                  # column ascending, then bin ascending
    counts = mask.sum(axis=0).astype(np.uint32)
    offs = np.zeros(A + 1, np.uint32)
    offs[1:] = np.cumsum(counts)
    a = (col - int(scroll)) % A
    theta = np.float32(theta_min) + a.astype(np.float32) * np.float32(theta_inc)
    r = ((b.astype(np.float64) + 0.5) * float(resolution)).astype(np.float32)
    pts = np.zeros(len(col), POINT_DTYPE)
    pts["x"] = r * np.cos(theta)
    pts["y"] = r * np.sin(theta)
    pts["intensity"] = img[b, col].astype(np.float32)
    pts["column"] = col
    pts["bin"] = b
    return pts, offs


def cartesian(img, width, pixel_size, bilinear=True, scroll=0, theta_min=0.0, theta_inc=-2 * np.pi / 400, resolution=0.0438,
              with_cells=False):
    """one polar image [n_cells][n_angles] -> uint8 [width][width]; with_cells (nearest): also the (bin, azimuth) each pixel
    read, and whether it lies past the last bin"""
    img = np.asarray(img)
    N, A = img.shape
    f32 = np.float32
    cc = f32(width - 1) * f32(0.5)
    ii, jj = np.meshgrid(np.arange(width, dtype=np.float32), np.arange(width, dtype=np.float32), indexing="ij")
    x = (cc - ii) * f32(pixel_size)
    y = (cc - jj) * f32(pixel_size)
    rho = np.sqrt(x * x + y * y)
    phi = np.arctan2(y, x)
    v = rho / f32(resolution) - f32(0.5)
    outside = ~(v <= f32(N) - f32(0.5))
    v = np.maximum(v, f32(0.0))
    na = f32(A)
    u = np.fmod((phi - f32(theta_min)) / f32(theta_inc), na)
    u = np.where(u < 0, u + na, u).astype(np.float32)
    u = np.where(u >= na, u - na, u).astype(np.float32)

    def z(b, a):
        return img[np.clip(b, 0, N - 1), (a + int(scroll) % A) % A].astype(np.float32)

    if not bilinear:
        a = np.rint(u).astype(np.int64) % A
        b = np.minimum(np.rint(v).astype(np.int64), N - 1)
        out = z(b, a)
        if with_cells:
            return np.clip(np.where(outside, 0, out), 0, 255).astype(np.uint8), np.clip(b, 0, N - 1), a, outside
    else:
        a0 = np.minimum(np.floor(u).astype(np.int64), A - 1)
        a1 = (a0 + 1) % A
        fu = (u - a0.astype(np.float32)).astype(np.float32)
        b0 = np.floor(v).astype(np.int64)
        b1 = np.minimum(b0 + 1, N - 1)
        fv = (v - b0.astype(np.float32)).astype(np.float32)
        one = f32(1.0)
        p0 = (one - fu) * z(b0, a0) + fu * z(b0, a1)
        p1 = (one - fu) * z(b1, a0) + fu * z(b1, a1)
        out = np.rint((one - fv) * p0 + fv * p1)
    out = np.clip(np.where(outside, 0, out), 0, 255)
    return out.astype(np.uint8)
