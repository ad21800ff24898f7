"""The inputs of the exact noise tests of k_column, shared by their GPU half (tests/test_gpu_column_noise.py) and their host half
(tests/test_column_noise_host.py), and a numpy restatement of the two steps the host half needs: the replay of an echo stream
into the slice (RadarCPU.cpp:402-450) and the noise amplitude law (:497-512) with its fourth power in both forms.

Everything here is a function of its arguments and of fixed seeds: both halves see the same streams."""
import math

import numpy as np

from test_gpu_column import TRI9, Seg, denoiser, echoes, strengths

N_ANGLES = 400
MB64 = denoiser(3, 64, 25)
DENOISERS = {"fmax": {}, "tri9": TRI9, "mb64": MB64}

# noise offsets, all finite and inside int (the reference's (int)floor is undefined beyond): 0; a lattice point at bin 0; the X wrap
# 255 -> 0 within the first bins at either scale; negative ones (floor, not truncation); a fraction that is a multiple of 1/64;
# the largest odd f32.  For the uniform stream, whose seed is (uint32_t)(int)rnd, also a negative non-integer and the largest
# f32 below 2^31.
OFFSETS = [0.0, 7.0, 255.96875, 511.9875, -0.5, -256.25, 999.984375, 16777215.0]
OFFSETS_UNIFORM = OFFSETS + [-3.7, 2147483520.0]


def offsets_of(noise):
    return np.float32(OFFSETS_UNIFORM if noise == 1 else OFFSETS)


# (az_begin, scroll, n_loc): image column = (scroll + azimuth) % 400.  Together they hold the columns 0, 5 (col * 0.2 = 1.0), 20
# (col * 0.05 = 1.0), 100 and 399, the wrap 399 -> 0 inside a block, and blocks with scroll > 0 and az_begin > 0.
LAYOUTS = [(0, 0, 6), (15, 5, 6), (394, 5, 6), (98, 0, 3)]


def layout_columns(layout):
    az_begin, scroll, n_loc = layout
    return [(scroll + az_begin + k) % N_ANGLES for k in range(n_loc)]


PEAK = 3.0          # dyadic columns: strengths k/16 * PEAK, k = 1 .. 16, and the peak itself


def dyadic(rs, n):
    """n strengths k/16 of PEAK.  With energy_max = 0.5 a bin's signal / max_val is k/32 exactly and 1 - k/32 has five significant
    bits: its fourth power is exact in f64 whichever way it is formed."""
    return (rs.randint(1, 17, n) / 16.0 * PEAK).astype(np.float32)


def column_kinds(n_cells, seed):
    """name -> Seg, for the config of `den_of(name)`.  The three kinds of test_gpu_column.test_noise: echoes in one 64-bin tile only,
    echoes in every tile, tiles whose only non-zero bin is their last; one echo; bin 0 alone and the last bin alone; and, under
    tri9, a window that rises and falls back to exactly 0.0f, alone and beside a tile that keeps its echoes."""
    rs = np.random.RandomState(seed)
    n_tiles = (n_cells + 63) // 64
    out = {}

    def seg(cells, strs):
        cells = np.asarray(cells, np.int64)
        strs = np.asarray(strs, np.float32)
        keep = (cells >= 0) & (cells < n_cells)
        s = echoes(cells[keep], strs[keep])
        if len(s):
            s["strength"][0] = PEAK                     # the column's peak is PEAK whatever the draw
        return Seg(s)
    t = rs.randint(0, n_tiles)
    out["one_tile"] = seg(rs.randint(64 * t + 8, 64 * t + 56, 40) % n_cells, dyadic(rs, 40))
    starts = np.arange(0, n_cells, 64)
    every = np.concatenate([starts + rs.randint(0, 64) % np.minimum(64, n_cells - starts), rs.randint(0, n_cells, 30)])
    out["every_tile"] = seg(every, dyadic(rs, len(every)))
    last = np.minimum(64 * np.arange(n_tiles) + 63, n_cells - 1)[::2 if n_tiles > 2 else 1]          # (a ragged tile: its last bin)
    out["last_bin_of_tiles"] = seg(last, dyadic(rs, len(last)))
    out["one_echo"] = seg([n_cells // 2], [PEAK])
    out["bin_0"] = seg([0], [PEAK])
    out["last_bin"] = seg([n_cells - 1], [PEAK])
    c = min(n_cells - 1, 64 * (n_tiles // 2) + 20)
    out["falls_to_zero"] = Seg(echoes([c, c], [2.0, -2.0]))
    far = (c + n_cells // 2) % n_cells                  # (its window does not reach c's: the column is 1 bin or 63 and more)
    out["falls_to_zero_beside_echoes"] = Seg(echoes([c, far, c, far], [2.0, 0.75, -2.0, 1.5]))
    return out


def den_of(kind):
    """the dyadic kinds run without a denoiser (the fmaxf path); a bin can only fall back to zero under one"""
    return TRI9 if kind.startswith("falls_to_zero") else {}


def random_columns(seed, n_cells):
    """step 3: columns of arbitrary strengths (the log-uniform draw of test_gpu_column.strengths), 3 to 300 echoes"""
    rs = np.random.RandomState(seed)
    segs = []
    for n in (3, 40, 300):
        segs.append(Seg(echoes(rs.randint(0, n_cells, n), strengths(rs, n))))
    clustered = rs.randint(0, min(n_cells, 30), 60) + rs.randint(0, max(n_cells - 30, 1))
    segs.append(Seg(echoes(clustered, strengths(rs, 60))))
    return segs


# step 3: (denoiser, n_cells) -> seed.  tests/test_column_noise_host.py proves for each that pow(x, 4.0) and (x * x) * (x * x)
# narrow to the same f32 in every non-empty bin of random_columns(seed, n_cells).
RANDOM_SEEDS = {(den, n_cells): 300 + 10 * k + j for k, den in enumerate(sorted(DENOISERS)) for j, n_cells in enumerate((200, 513))}


# ---------------------------------------------------------------------------------------------------------------------------
def replay(cfg, smear, mode, stream):
    """RadarCPU.cpp:402-450 in numpy: (slice f32 [n_cells], max_val f32) of one ordered stream.  smear: the denoiser's weights
    (oracle.make_denoiser(kind, width, mode, rescale=True)) or None."""
    n_cells = cfg.n_cells
    sl = np.zeros(n_cells, np.float32)
    max_val = np.float32(0.0)
    for cell, s in zip(stream["cell"].tolist(), stream["strength"]):
        if not 0 <= cell < n_cells:
            continue
        if smear is None:
            sl[cell] = max(sl[cell], s)
            max_val = max(max_val, sl[cell])
            continue
        first = cell - mode
        lo, hi = max(first, 1), min(first + len(smear), n_cells)          # glob_id > 0 (:424)
        if hi <= lo:
            continue
        w = smear[lo - first:hi - first].astype(np.float64)
        sl[lo:hi] = (sl[lo:hi].astype(np.float64) + np.float64(s) * w).astype(np.float32)
        max_val = max(max_val, sl[lo:hi].max())
    return sl, np.float32(max_val)


def smear_of(oracle, cfg):
    if not cfg.signal_denoising:
        return None, 0
    name = {1: "triangular", 2: "gaussian", 3: "mb"}[cfg.signal_denoising]
    width = getattr(cfg, "signal_denoising_%s_width" % name)
    mode = int(getattr(cfg, "signal_denoising_%s_mode" % name) * width)
    return oracle.make_denoiser(cfg.signal_denoising, width, mode, rescale=True), mode


def fourth_powers(cfg, sl, max_val):
    """signal_ = 1 - signal / max_val of every non-empty bin (RadarCPU.cpp:497-508) and the f32 its fourth power narrows to: by
    numpy's power, by libm's pow -- what the oracle calls -- and by two squarings -- what the kernel does."""
    with np.errstate(all="ignore"):
        signal = sl[sl != 0] * np.float32(cfg.energy_max)
        q = (signal - np.float32(0.0)) / np.float32(max_val - np.float32(0.0))          # f32 division
        x = (1.0 - q.astype(np.float64)).astype(np.float32).astype(np.float64)
        by_power = np.power(x, 4.0).astype(np.float32)
        by_libm = np.array([math.pow(v, 4.0) for v in x.tolist()], np.float64).astype(np.float32)
        sq = x * x
        by_squaring = (sq * sq).astype(np.float32)
    return x, by_power, by_libm, by_squaring
