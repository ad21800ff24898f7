"""numpy restatement of the label definition (include/radarays_mi355.h, rr_simulate_batch_provenance_device): one azimuth's ordered
echoes in, the two label columns out.  Deliberately literal -- a loop over echoes and taps, the f64 product rounded once to f32, the
64-bit key with its tie rule -- so that it can be checked by hand (tests/test_labels_host.py) and the kernel against it
(tests/test_gpu_labels.py)."""
import numpy as np

NONE = 0xFFFFFFFF


def weights(cfg, oracle):
    """(w f32 [W], mode) the column step uses under cfg: the oracle's rescaled denoiser (RadarCPU.cpp:48-93); no denoiser: ([1], 0)"""
    kind = int(cfg.signal_denoising)
    if kind <= 0:
        return np.ones(1, np.float32), 0
    name = {1: "triangular", 2: "gaussian", 3: "mb"}[kind]
    width = int(getattr(cfg, "signal_denoising_%s_width" % name))
    if width <= 0:
        return np.ones(1, np.float32), 0
    mode = int(float(getattr(cfg, "signal_denoising_%s_mode" % name)) * width)
    return oracle.make_denoiser(kind, width, mode, rescale=True), mode


def term(strength, weight):
    """(float)((double)strength * (double)weight): exact product, one rounding"""
    with np.errstate(all="ignore"):
        return np.float32(np.float64(np.float32(strength)) * np.float64(np.float32(weight)))


def label_column(cells, strengths, infos, faces, n_cells, w, mode):
    """-> (label uint32 [n_cells], face uint32 [n_cells]) of one azimuth"""
    w = np.asarray(w, np.float32)
    W = len(w)
    key = [0] * n_cells
    for k in range(len(cells)):
        c = int(cells[k])
        if not 0 <= c < n_cells:
            continue
        for t in range(W):
            g = c - mode + t
            if not 0 < g < n_cells:            # bin 0 is never written
                continue
            v = term(strengths[k], w[t])
            if not (np.isfinite(v) and v > 0):
                continue
            kk = (int(np.float32(v).view(np.uint32)) << 32) | (0xFFFFFFFF - k)
            if kk > key[g]:
                key[g] = kk
    lab = np.full(n_cells, NONE, np.uint32)
    fac = np.full(n_cells, NONE, np.uint32)
    for g in range(n_cells):
        if key[g]:
            k = 0xFFFFFFFF - (key[g] & 0xFFFFFFFF)
            lab[g], fac[g] = infos[k], faces[k]
    return lab, fac


def label_column_fast(cells, strengths, infos, faces, n_cells, w, mode):
    """the same columns, vectorised over echoes (one pass per tap): for streams of thousands of echoes under wide windows"""
    w = np.asarray(w, np.float32)
    cells = np.asarray(cells, np.int64)
    n = len(cells)
    key = np.zeros(n_cells, np.uint64)
    ok = (cells >= 0) & (cells < n_cells)
    idx = np.uint64(0xFFFFFFFF) - np.arange(n, dtype=np.uint64)
    with np.errstate(all="ignore"):
        for t in range(len(w)):
            g = cells - mode + t
            v = (np.asarray(strengths, np.float32).astype(np.float64) * np.float64(w[t])).astype(np.float32)
            m = ok & (g > 0) & (g < n_cells) & np.isfinite(v) & (v > 0)
            if m.any():
                np.maximum.at(key, g[m], (v[m].view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx[m])
    lab = np.full(n_cells, NONE, np.uint32)
    fac = np.full(n_cells, NONE, np.uint32)
    hit = key != 0
    k = (np.uint64(0xFFFFFFFF) - (key[hit] & np.uint64(0xFFFFFFFF))).astype(np.int64)
    lab[hit], fac[hit] = np.asarray(infos, np.uint32)[k], np.asarray(faces, np.uint32)[k]
    return lab, fac


def label_planes(echoes, counts, n_cells, w, mode, scroll, fast=True):
    """echoes [n_angles][stride] (fields cell, strength, face, info), counts [n_angles] -> (labels, faces) uint32 [n_cells][n_angles] in
    image layout: azimuth a in column (scroll + a) % n_angles"""
    A = len(counts)
    lab = np.zeros((n_cells, A), np.uint32)
    fac = np.zeros((n_cells, A), np.uint32)
    f = label_column_fast if fast else label_column
    for a in range(A):
        e = echoes[a, :int(counts[a])]
        col = (scroll + a) % A
        lab[:, col], fac[:, col] = f(e["cell"], e["strength"], e["info"], e["face"], n_cells, w, mode)
    return lab, fac


def pack_info(obj, pas, kind):
    return np.uint32((int(obj) & 0xFFFFFF) | (int(pas) << 24) | (int(kind) << 28))
