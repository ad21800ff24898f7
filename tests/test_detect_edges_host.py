"""The detectors and the Cartesian resampler at their tiling edges, without a GPU: the case tables of tests/test_gpu_detect_edges.py
and the premises its comparison rests on, proved on the numpy restatement (tests/detect_ref.py) alone.

What the kernels of rr_detect.hip do that makes these the edges (restated here, not imported):
  k_detect<TW, METHOD, EMIT>  512 threads per workgroup, a tile of TW columns, a column owned by TPC = 512 / TW threads (32 or 128),
                              thread k owning bins [k * chunk, (k + 1) * chunk), chunk = ceil(n_cells / TPC).  TW is 16 while
                              align16(TW * n_cells) + 2048 (+ TW * 512 for k-strongest) + 256 fits 64 KB, else 4: 16 up to 3440 cells
                              for k-strongest and up to 3952 for CA-CFAR.  Rows of a tile are loaded as TW-byte words when
                              n_angles % TW == 0 and the image base is TW-aligned, else byte by byte with a zero-filled last tile.
  k_detect_scan               one wave walks the azimuths 64 at a time.
  k_cartesian                 at most 8192 workgroups of 256 threads x 4 pixels: beyond 8,388,608 output pixels the grid-stride loop takes
                              a second trip; uchar4 stores when the output base is 4-byte aligned, else byte stores.

Boundaries the tables cover:
  column heights 1, 2, 31, 32, 33, 127, 128, 129 (TPC = 32: empty chunks, one cell either side of a multiple of TPC), 3440 / 3441 and
  3952 / 3953 (the tile-width switch of either method), 3967, 3968, 3969 (TW = 4: one cell either side of a multiple of 128), 8192 (the
  ABI's maximum); azimuth counts 1, 15, 16, 17, 63, 65, 129 and 4099 (65 rounds of the scan, no multiple of 4); TW = 4 with byte loads
  (3953 x 37); scroll 0 and n_angles - 1; CA-CFAR windows reaching past the column on both sides (n = 0: no detection), on one side only
  for every bin, guard and train at 1024, (2, 16) at 8 cells, cfar_scale = 0; k-strongest at k = 1, k = 64 and k = n_cells with
  min_intensity 0 and 255, min_bin = n_cells - 1, ties at the threshold that straddle chunk boundaries with larger values in between, and
  a threshold value whose partner in the same histogram word holds more than 1,000 cells; counter-clockwise geometry with a non-zero
  theta_min.  Cartesian: a second grid trip (2 x 2049 x 2049 pixels), widths 3 and 5, 1, 2 and 3 azimuths, 1 cell, theta_inc > 0,
  theta_min -pi and 0.3, scroll n_angles - 1, output bases 1, 2 and 3 bytes past an aligned one.
Image bases 1, 4 and 8 bytes past an aligned allocation belong to the GPU file alone (UNALIGNED below names their shapes).

Not covered: more than 4099 azimuths (the ABI allows 65536), frames counts beyond 3, guard + train windows of one side only at TW = 4
(2 * 1024 + 2 cells is less than 3953), and widths above 2049."""
import functools
from collections import namedtuple

import numpy as np
import pytest

import detect_ref as R
from radarays_ros_amd import params
from test_gpu_detect import synthetic

TB, LDS_MAX = 512, 65536
GRID_PIXELS = 8192 * 256 * 4          # one trip of k_cartesian's grid


def align16(x):
    return (x + 15) & ~15


def detect_lds(tw, method, n_cells):
    return align16(tw * n_cells) + 2048 + (tw * 512 if method == 1 else 0) + 256


def tile_width(method, n_cells):
    return 16 if detect_lds(16, method, n_cells) <= LDS_MAX else 4


def chunk_of(method, n_cells):
    """bins per thread of a column"""
    tpc = TB // tile_width(method, n_cells)
    return -(-n_cells // tpc)


CFAR = dict(method=0, guard_cells=2, train_cells=16, k=12, min_intensity=1, min_bin=0, cfar_scale=3.0)
KSTR = dict(CFAR, method=1)


def cfar(**kw):
    return dict(CFAR, **kw)


def kstr(**kw):
    return dict(KSTR, **kw)


# expect: "some" (every case means to detect something), "none" (no training cell anywhere: zero detections), "tie", "shared"
# craft: the name of a crafted third frame (CRAFT below); ccw: theta_inc = +2 pi / n_angles
Det = namedtuple("Det", "name family n_cells n_angles scroll det expect craft ccw theta_min")
DET_CASES = []


def _det(name, family, n_cells, n_angles, det, expect="some", scroll=0, craft=None, ccw=False, theta_min=0.0):
    det = dict(det, k=min(det["k"], n_cells))                 # the ABI wants k <= n_cells of CA-CFAR calls too
    DET_CASES.append(Det(name, family, n_cells, n_angles, scroll, det, expect, craft, ccw, theta_min))


HEIGHTS = (1, 2, 31, 32, 33, 127, 128, 129, 3440, 3441, 3952, 3953, 3967, 3968, 3969, 8192)
for _n in HEIGHTS:
    _na = 48 if _n <= 129 else 32 if _n < 8192 else 16
    _det("h%d-cfar" % _n, "heights", _n, _na, CFAR, "some" if _n > 3 else "none")       # G = 2: 3 cells or fewer train on nothing
    _det("h%d-k12" % _n, "heights", _n, _na, kstr(k=min(12, _n)))
_det("h1-cfar_g0t1", "heights", 1, 48, cfar(guard_cells=0, train_cells=1), "none")
_det("h2-cfar_g0t1", "heights", 2, 48, cfar(guard_cells=0, train_cells=1))
for _na in (1, 15, 16, 17, 63, 65, 129, 4099):
    _det("a%d-cfar" % _na, "azimuths", 40, _na, CFAR)
    _det("a%d-k12" % _na, "azimuths", 40, _na, KSTR)
_det("tw4bytes-cfar", "tw4-bytes", 3953, 37, CFAR)
_det("tw4bytes-k12-scroll36", "tw4-bytes", 3953, 37, KSTR, scroll=36)
_det("scroll47-cfar", "scroll", 33, 48, CFAR, scroll=47)
_det("scroll47-k12", "scroll", 33, 48, KSTR, scroll=47)
_det("scroll31-tw4-k12", "scroll", 3968, 32, KSTR, scroll=31)

P16, P4 = (300, 48), (3968, 16)                                  # the parameter edges: one TW = 16 shape, one TW = 4 shape
_det("g1024t1024-300", "cfar-windows", 300, 48, cfar(guard_cells=1024, train_cells=1024), "none")
_det("g1024t1-300", "cfar-windows", 300, 48, cfar(guard_cells=1024, train_cells=1), "none")
_det("g1024t1024-1500-one-side", "cfar-windows", 1500, 16, cfar(guard_cells=1024, train_cells=1024))
_det("g1024t1024-3968", "cfar-windows", 3968, 16, cfar(guard_cells=1024, train_cells=1024))
_det("g2t16-8cells", "cfar-windows", 8, 48, CFAR)
for _s, (_n, _na) in (("tw16", P16), ("tw4", P4)):
    _det("g0t1024-" + _s, "cfar-windows", _n, _na, cfar(guard_cells=0, train_cells=1024))
    if _n > 1025:
        _det("g1024t1-" + _s, "cfar-windows", _n, _na, cfar(guard_cells=1024, train_cells=1))
    _det("scale0-" + _s, "cfar-scale0", _n, _na, cfar(cfar_scale=0.0))
    for _k in (1, 64, _n):
        for _mi in (0, 255):
            _det("k%d-min%d-%s" % (_k, _mi, _s), "k-and-min-intensity", _n, _na, kstr(k=_k, min_intensity=_mi))
    _det("minbin-last-cfar-" + _s, "min-bin", _n, _na, cfar(min_bin=_n - 1))
    _det("minbin-last-k12-" + _s, "min-bin", _n, _na, kstr(min_bin=_n - 1))
    _det("ties-" + _s, "ties", _n, _na, KSTR, "tie", craft="ties")
    _det("ccw-cfar-" + _s, "ccw", _n, _na, CFAR, scroll=5, ccw=True, theta_min=0.3)
    _det("ccw-k12-" + _s, "ccw", _n, _na, KSTR, scroll=5, ccw=True, theta_min=0.3)
_det("shared-hi-tw16", "shared-word", 3440, 16, KSTR, "shared", craft="shared")            # threshold 101, its partner 100
_det("shared-lo-tw16", "shared-word", 3440, 16, kstr(k=1600), "shared", craft="shared")    # threshold 100, its partner 101
_det("shared-hi-tw4", "shared-word", 4000, 8, KSTR, "shared", craft="shared")
_det("shared-lo-tw4", "shared-word", 4000, 8, kstr(k=1600), "shared", craft="shared")
DET_IDS = [c.name for c in DET_CASES]

# image bases past an aligned allocation (device form, tests/test_gpu_detect_edges.py): at 4 bytes TW = 16 falls to byte loads and
# TW = 4 keeps its words; 48 azimuths are a multiple of both widths, so only the base decides
UNALIGNED_OFFSETS = (1, 4, 8)
UNALIGNED = [c for c in DET_CASES if c.name in ("ties-tw16", "h3953-cfar", "h3953-k12")]
UNALIGNED.append(Det("u-cfar-tw16", "unaligned", 300, 48, 0, CFAR, "some", None, False, 0.0))
assert all(c.n_angles % tile_width(c.det["method"], c.n_cells) == 0 for c in UNALIGNED)
assert {tile_width(c.det["method"], c.n_cells) for c in UNALIGNED} == {4, 16}

TIE_VALUE, SHARED_LO = 100, 100


def _ties(c):
    """every column: k // 2 + 1 cells above TIE_VALUE, k cells equal to it (so k // 2 + 1 of those are left over), the rest below it,
    all at random bins"""
    rs = np.random.RandomState(c.n_cells)
    k = c.det["k"]
    img = rs.randint(0, 50, (c.n_cells, c.n_angles)).astype(np.uint8)
    n_big = k // 2 + 1
    for col in range(c.n_angles):
        p = rs.permutation(c.n_cells)
        img[p[:n_big], col] = rs.randint(150, 256, n_big)
        img[p[n_big:n_big + k], col] = TIE_VALUE
    return img


def _shared(c):
    """every column: 5 cells of 200, 1,500 of SHARED_LO, 1,500 of SHARED_LO + 1 (one histogram word), the rest below 50"""
    rs = np.random.RandomState(c.n_cells + 1)
    img = rs.randint(0, 50, (c.n_cells, c.n_angles)).astype(np.uint8)
    for col in range(c.n_angles):
        p = rs.permutation(c.n_cells)
        img[p[:5], col] = 200
        img[p[5:1505], col] = SHARED_LO
        img[p[1505:3005], col] = SHARED_LO + 1
    return img


CRAFT = {"ties": _ties, "shared": _shared}


def frames(c):
    """a noisy frame with sparse peaks, the all-255 frame (everything ties) and the case's crafted frame, if it has one"""
    x = synthetic(5, c.n_cells, c.n_angles, seed=c.n_cells + c.n_angles)[[0, 4]]
    if c.craft:
        x = np.concatenate([x, CRAFT[c.craft](c)[None]])
    return np.ascontiguousarray(x)


def geometry(c):
    """what tests/test_gpu_detect.py's geometry() reads back from a context configured for the case"""
    inc = (2.0 if c.ccw else -2.0) * np.pi / c.n_angles
    return dict(scroll=c.scroll, theta_min=float(np.float32(c.theta_min)), theta_inc=float(np.float32(inc)),
                resolution=params.kaist_preset(n_cells=c.n_cells).resolution)


def config_kw(c):
    """the keywords of native.Context.set_config for the case's geometry"""
    return dict(theta_min=c.theta_min, theta_inc=2.0 * np.pi / c.n_angles if c.ccw else None) if c.ccw or c.theta_min else {}


@functools.lru_cache(maxsize=None)
def _want(name):
    c = DET_CASES[DET_IDS.index(name)] if name in DET_IDS else next(u for u in UNALIGNED if u.name == name)
    return tuple(R.detect_frame(img, **c.det, **geometry(c)) for img in frames(c))


def want(c):
    """the restatement's (points, offsets) of every frame of the case, computed once"""
    return _want(c.name)


def _threshold(col, det):
    """(threshold value, cells above it among the candidates) of one column under k-strongest"""
    i = np.arange(len(col))
    cand = np.sort(col[(col >= det["min_intensity"]) & (i >= det["min_bin"])].astype(int))[::-1]
    assert len(cand) > det["k"]
    t = int(cand[det["k"] - 1])
    return t, int((cand > t).sum())


def test_case_names_are_unique_and_inside_the_abi():
    assert len(set(DET_IDS)) == len(DET_IDS)
    for c in DET_CASES + UNALIGNED:
        d = c.det
        assert 1 <= c.n_cells <= 8192 and 1 <= c.n_angles <= 65536 and 0 <= c.scroll < c.n_angles
        assert 0 <= d["guard_cells"] <= 1024 and 1 <= d["train_cells"] <= 1024 and 1 <= d["k"] <= c.n_cells
        assert 0 <= d["min_intensity"] <= 255 and 0 <= d["min_bin"] < c.n_cells and d["cfar_scale"] >= 0
    assert {c.n_cells for c in DET_CASES if c.family == "heights"} == set(HEIGHTS)
    assert {c.n_angles for c in DET_CASES if c.family == "azimuths"} == {1, 15, 16, 17, 63, 65, 129, 4099}
    assert all(c.scroll == c.n_angles - 1 for c in DET_CASES if c.family == "scroll")


def test_tile_width_switches_where_the_kernel_file_says():
    assert [tile_width(1, n) for n in (3440, 3441)] == [16, 4]
    assert [tile_width(0, n) for n in (3952, 3953)] == [16, 4]
    assert detect_lds(16, 1, 3440) == LDS_MAX and detect_lds(16, 0, 3952) == LDS_MAX
    assert detect_lds(4, 1, 8192) < LDS_MAX and detect_lds(4, 0, 8192) < LDS_MAX
    got = {c.name: tile_width(c.det["method"], c.n_cells) for c in DET_CASES}
    for n in HEIGHTS:
        assert got["h%d-cfar" % n] == (16 if n <= 3952 else 4) and got["h%d-k12" % n] == (16 if n <= 3440 else 4), n
    # one cell either side of a multiple of TPC: the last chunk is ragged, or whole chunks are empty
    for n, tw in ((31, 16), (32, 16), (33, 16), (127, 16), (128, 16), (129, 16), (3967, 4), (3968, 4), (3969, 4)):
        assert tile_width(0, n) == tile_width(1, n) == tw
    assert 3968 % 128 == 0 and 128 % 32 == 0 and 32 % 32 == 0
    assert all(tile_width(c.det["method"], c.n_cells) == 4 and c.n_angles % 4 for c in DET_CASES if c.family == "tw4-bytes")
    assert all(tile_width(c.det["method"], c.n_cells) == (16 if c.name.endswith("tw16") else 4) for c in DET_CASES
               if c.name.endswith(("tw16", "tw4")))
    print("tile width: k-strongest 3440 -> %d, 3441 -> %d; CA-CFAR 3952 -> %d, 3953 -> %d; LDS at the last 16-wide heights %d and %d B"
          % (tile_width(1, 3440), tile_width(1, 3441), tile_width(0, 3952), tile_width(0, 3953), detect_lds(16, 1, 3440), detect_lds(16, 0, 3952)))


@pytest.mark.parametrize("family", sorted({c.family for c in DET_CASES}))
def test_cases_detect_where_they_mean_to(family):
    line = []
    for c in (c for c in DET_CASES if c.family == family):
        totals = [int(offs[-1]) for _, offs in want(c)]
        if c.expect == "none":
            assert totals == [0] * len(totals), c.name
            i = np.arange(c.n_cells)
            G, T = c.det["guard_cells"], c.det["train_cells"]
            assert np.all(i - G - 1 < 0) and np.all(i + G + 1 > c.n_cells - 1), c.name       # no bin has a training cell
        else:
            assert sum(totals) > 0 and (totals[0] > 0 or c.det["min_intensity"] == 255), c.name     # (frame 0 may hold no 255)
            if c.craft:
                assert totals[-1] > 0, c.name
        line.append("%s %s" % (c.name, totals))
    print("%s: detections per frame: %s" % (family, "; ".join(line)))


def test_one_sided_windows_are_one_sided():
    c = DET_CASES[DET_IDS.index("g1024t1024-1500-one-side")]
    i = np.arange(c.n_cells)
    G = c.det["guard_cells"]
    left, right = i - G - 1 >= 0, i + G + 1 <= c.n_cells - 1
    assert not np.any(left & right) and left.any() and right.any() and np.any(~left & ~right)
    pts = want(c)[0][0]
    assert np.any(left[pts["bin"]]) and np.any(right[pts["bin"]])        # detections under a left-only and under a right-only window


@pytest.mark.parametrize("name", [c.name for c in DET_CASES if c.expect == "tie"])
def test_ties_straddle_chunks_with_larger_values_between(name):
    c = DET_CASES[DET_IDS.index(name)]
    img = frames(c)[-1]
    chunk = chunk_of(1, c.n_cells)
    spread = []
    for col in range(c.n_angles):
        z = img[:, col].astype(int)
        t, above = _threshold(img[:, col], c.det)
        quota = c.det["k"] - above
        at = np.nonzero(z == t)[0]
        assert t == TIE_VALUE and 0 < quota < len(at), (col, t, quota, len(at))
        chunks = np.unique(at // chunk)
        assert len(chunks) >= 3, (col, chunks)
        assert np.any(z[at[0]:at[-1]] > t), col                              # a larger value between two of them
        taken, left_out = at[:quota], at[quota:]
        assert np.any(z[taken[0]:left_out[-1]] > t), col
        spread.append(len(chunks))
        got = want(c)[-1][0]
        mine = got[got["column"] == col]
        assert np.array_equal(np.sort(mine["bin"][mine["intensity"] == t]), taken), col   # the restatement takes the first by bin
    print("%s: chunk of %d bins, ties of every column lie in %d..%d chunks, quota %d of %d" % (name, chunk, min(spread), max(spread), quota, len(at)))


@pytest.mark.parametrize("name", [c.name for c in DET_CASES if c.expect == "shared"])
def test_the_threshold_shares_its_histogram_word(name):
    c = DET_CASES[DET_IDS.index(name)]
    img = frames(c)[-1]
    for col in range(c.n_angles):
        t, _ = _threshold(img[:, col], c.det)
        w = t >> 1
        n_lo, n_hi = int((img[:, col] == 2 * w).sum()), int((img[:, col] == 2 * w + 1).sum())
        assert n_lo > 1000 and n_hi > 1000, (col, n_lo, n_hi)
        assert t == (SHARED_LO + 1 if "-hi-" in name else SHARED_LO), (col, t)
    print("%s: threshold %d, %d cells of %d and %d of %d in its word" % (name, t, n_lo, 2 * w, n_hi, 2 * w + 1))


# ---- Cartesian --------------------------------------------------------------------------------------------------------------------
# out_offset: the output base lies that many bytes past an aligned one (device form only)
Cart = namedtuple("Cart", "name width n_frames n_cells n_angles scroll bilinear ccw theta_min out_offset")
CART_CASES = []


def _cart(name, width, n_frames=3, n_cells=64, n_angles=400, scroll=0, bilinear=False, ccw=False, theta_min=0.0, out_offset=0):
    CART_CASES.append(Cart(name, width, n_frames, n_cells, n_angles, scroll, bilinear, ccw, theta_min, out_offset))


for _b in (False, True):
    _s = "-bilinear" if _b else "-nearest"
    _cart("big" + _s, 2049, n_frames=2, bilinear=_b)
    _cart("w3" + _s, 3, bilinear=_b)
    _cart("w5" + _s, 5, bilinear=_b)
    for _na in (1, 2, 3):
        _cart("a%d%s" % (_na, _s), 65, n_angles=_na, bilinear=_b)
    _cart("one-cell" + _s, 33, n_cells=1, bilinear=_b)
    _cart("ccw" + _s, 129, ccw=True, bilinear=_b)
    _cart("theta-min-pi" + _s, 129, theta_min=-np.pi, bilinear=_b)
    _cart("theta-min-0.3-ccw" + _s, 129, theta_min=0.3, ccw=True, bilinear=_b)
    _cart("theta-min-0.3" + _s, 129, theta_min=0.3, bilinear=_b)
    _cart("scroll399" + _s, 129, scroll=399, bilinear=_b)
for _o in (1, 2, 3):
    _cart("out+%d" % _o, 33, out_offset=_o, bilinear=_o == 2)       # 3 x 33 x 33 pixels: no multiple of 4, the last group is ragged
CART_IDS = [c.name for c in CART_CASES]


def pixel_size(c):
    """the image reaches a little past the last bin"""
    return 2 * c.n_cells * params.kaist_preset(n_cells=c.n_cells).resolution / c.width


def cart_frames(c):
    imgs = synthetic(c.n_frames, c.n_cells, c.n_angles, seed=c.width)
    imgs[0] = np.random.RandomState(1).randint(0, 256, imgs[0].shape)        # noise: every rounding shows
    return imgs


@functools.lru_cache(maxsize=None)
def cart_want(name, f):
    """the restatement of frame f: the image (bilinear), or (image, bin, azimuth, outside) (nearest)"""
    c = CART_CASES[CART_IDS.index(name)]
    img = cart_frames(c)[f]
    if c.bilinear:
        return R.cartesian(img, c.width, pixel_size(c), True, **geometry(c))
    return R.cartesian(img, c.width, pixel_size(c), False, with_cells=True, **geometry(c))


def test_the_big_case_takes_a_second_grid_trip_that_is_not_all_zeros():
    for name in ("big-nearest", "big-bilinear"):
        c = CART_CASES[CART_IDS.index(name)]
        total = c.n_frames * c.width * c.width
        assert GRID_PIXELS == 8388608 < total < 2 * GRID_PIXELS
        f, rem = divmod(GRID_PIXELS, c.width * c.width)
        assert f == c.n_frames - 1
    out, b, a, outside = cart_want("big-nearest", f)
    trip = slice(rem, None)
    inside = ~outside.ravel()[trip]
    lit = inside & (out.ravel()[trip] > 0)
    assert inside.sum() > 100 and lit.sum() > 100
    assert b.ravel()[trip][inside].max() == c.n_cells - 1                   # pixels of the trip reach the last bin
    assert np.any(cart_want("big-bilinear", f).ravel()[trip] > 0)
    print("big case: %d pixels, %d in the second grid trip (rows %d.. of frame %d), %d of them inside the last bin, %d non-zero"
          % (total, total - GRID_PIXELS, rem // c.width, f, int(inside.sum()), int(lit.sum())))


def test_cartesian_cases_read_the_image():
    """every case lights pixels in every frame, small widths included; the geometry cases differ from the default geometry"""
    line = []
    for c in CART_CASES:
        assert 1 <= c.width <= 8192 and 0 <= c.scroll < c.n_angles
        for f in range(c.n_frames):
            w = cart_want(c.name, f)
            img = w if c.bilinear else w[0]
            assert img.shape == (c.width, c.width) and img.any(), (c.name, f)
        line.append("%s %d" % (c.name, int((img > 0).sum())))
    for s in ("-nearest", "-bilinear"):
        plain = R.cartesian(cart_frames(CART_CASES[CART_IDS.index("ccw" + s)])[0], 129, pixel_size(CART_CASES[CART_IDS.index("ccw" + s)]),
                            s == "-bilinear", **geometry(CART_CASES[CART_IDS.index("ccw" + s)]._replace(ccw=False)))
        for name in ("ccw", "theta-min-pi", "theta-min-0.3", "theta-min-0.3-ccw", "scroll399"):
            w = cart_want(name + s, 0)
            assert np.mean((w if s == "-bilinear" else w[0]) != plain) > 0.5, name + s
    # 1, 2 and 3 azimuths: a1 wraps onto a0 or onto azimuth 0
    for na in (1, 2, 3):
        _, b, a, outside = cart_want("a%d-nearest" % na, 0)
        assert set(np.unique(a)) == set(range(na))
    print("cartesian: lit pixels of the last frame: " + "; ".join(line))
