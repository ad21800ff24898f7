"""The cases that hold the image metrics (rr_metrics.hip, k_score) to their tile, strip and alignment edges, and the proof that
each case reaches its edge, without a GPU.  tests/test_gpu_metrics_edges.py imports cases(), ssim_pairs() and hist_inputs() and runs
them on the library.

The case list is built from the kernels' own constants, read out of rr_metrics.hip: a change of a tile constant fails here
instead of quietly turning edge cases into interior ones.

- k_ssim works in tiles of kSsimTH x kSsimTW window positions.  The seam cases put out_h at TH - 1, TH, TH + 1 and 2 TH + 1 and
  out_w at TW - 1, TW, TW + 1 and 2 TW + 1 for windows 3, 7 and 15 (the corners of the product, not all of it).
- k_metrics_finish sums the SSIM partials in strides of its block: one partial fewer than a stride, a stride, two more.
- k_joint_hist walks strips of kHistStrip pixels: 15 pixels short of a strip, a strip, 1, 2 and 16 pixels past it, two strips,
  3 pixels past two.
- Both operands of hist_walk and k_score at byte offsets past aligned allocations.

What a mean can see.  The library returns the mean of S over the window positions, held to 1e-9.  A position whose S is 0
could go missing unnoticed, and so could one that is swapped for a neighbour with the same S.  Every SSIM case therefore runs on
four input pairs, and this file asserts with the per-position reference (metrics_ref.ssim_map) that every position has
|S| >= 0.01 in at least one pair and that every two positions adjacent across a tile seam, or at the last row or column, differ by
0.01 or more in at least one pair: 0.01 over at most 65 x 129 positions moves the mean by 1.2e-6, a thousand times the bound.
Pairs 0 and 1 are uniform noise in [40, 216) against itself plus uniform [-60, 60]; their windows of 7 and 15 all look alike
(neighbouring S differ by 0.001 .. 0.008), so pairs 2 and 3 mirror the image about mid-grey on every other row, and on every
other column: an odd window one step further holds one mirrored line more or fewer, and S moves by 0.05 or more."""
import collections
import os
import re

import numpy as np
import pytest

import metrics_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "radarays_ros_amd", "csrc", "rr_metrics.hip")

MAX_CELLS, MAX_ANGLES = 8192, 65536             # rr_set_config's limits
MAX_PIXELS = 400000                             # every case stays below this
VISIBLE = 0.01

SsimCase = collections.namedtuple("SsimCase", "win out_h out_w")
FinishCase = collections.namedtuple("FinishCase", "win n_cells n_angles n_blocks")
HistCase = collections.namedtuple("HistCase", "n_cells n_angles n_px what")

WINDOWS = (3, 7, 15)
# (multiples of the tile, pixels past them) of out_h and out_w: the four corners the seams need, and four more
SEAM_CORNERS = (((1, 0), (1, 0)), ((1, 1), (1, 1)), ((1, -1), (2, 1)), ((2, 1), (1, -1)),
                ((1, -1), (1, -1)), ((2, 1), (2, 1)), ((1, 1), (1, 0)), ((1, 0), (1, 1)))
# image shapes whose SSIM partial counts (win 7) are the finish stride - 1, the stride and the stride + 2
FINISH_SHAPES = ((2726, 135, -1), (4102, 71, 0), (2758, 135, 2))
# n_cells x n_angles, (strips, pixels past them), what the count exercises
HIST_SHAPES = ((4367, 15, (1, -15), "odd: image 1 is misaligned; a last group of 1 pixel"),
               (4095, 16, (1, 0), "exactly one strip"),
               (1, 65521, (1, 1), "one pixel in the second strip: byte tail only"),
               (362, 181, (1, 2), "two pixels past one strip"),
               (4096, 16, (1, 16), "16 pixels past one strip: one 16-byte group, no tail"),
               (8190, 16, (2, 0), "exactly two strips"),
               (627, 209, (2, 3), "three pixels past two strips"))
# shapes and (image stack, reference) byte offsets of the alignment cases
ALIGN_SHAPES = ((4095, 16), (362, 181))
ALIGN_OFFSETS = ((0, 1), (1, 0), (1, 1), (3, 5), (16, 0))


def image_shape(c):
    return c.out_h + c.win - 1, c.out_w + c.win - 1


def constants():
    """kHistStrip, kSsimTW, kSsimTH, kSsimTB and the stride of k_metrics_finish's sum over the partials, from the source"""
    src = open(SOURCE).read()
    k = {}
    for name in ("kHistStrip", "kSsimTW", "kSsimTH", "kSsimTB"):
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % name, src)
        assert m, name
        k[name] = int(m.group(1))
    m = re.search(r"for \(int b = t; b < n_blocks; b \+= (\d+)\)", src)
    assert m, "the loop of k_metrics_finish over the SSIM partials"
    k["finish_stride"] = int(m.group(1))
    return k


def ssim_blocks(n_cells, n_angles, win, k):
    return -(-(n_cells - win + 1) // k["kSsimTH"]) * -(-(n_angles - win + 1) // k["kSsimTW"])


def cases(k=None):
    """every case of tests/test_gpu_metrics_edges.py from the constants of rr_metrics.hip -> dict of lists"""
    k = k or constants()
    th, tw, strip = k["kSsimTH"], k["kSsimTW"], k["kHistStrip"]
    ssim = [SsimCase(w, mh * th + dh, mw * tw + dw) for w in WINDOWS for (mh, dh), (mw, dw) in SEAM_CORNERS]
    finish = [FinishCase(7, nc, na, k["finish_stride"] + d) for nc, na, d in FINISH_SHAPES]
    hist = [HistCase(nc, na, m * strip + d, what) for nc, na, (m, d), what in HIST_SHAPES]
    return {"ssim": ssim, "finish": finish, "hist": hist, "align": [(s, o) for s in ALIGN_SHAPES for o in ALIGN_OFFSETS]}


def case_id(c):
    if isinstance(c, SsimCase):
        return "w%d_%dx%d" % c
    if isinstance(c, FinishCase):
        return "%dx%d_%d_partials" % (c.n_cells, c.n_angles, c.n_blocks)
    return "%dx%d" % (c.n_cells, c.n_angles)


# ---- inputs -------------------------------------------------------------------------------------------------------------

def ssim_pair(shape, win, k):
    """input pair k of 4 for an image shape -> (image, reference); see the file's docstring"""
    rs = np.random.RandomState(7919 * win + 101 * shape[0] + 10 * shape[1] + k)
    ref = rs.randint(40, 216, shape)
    base = ref.copy()
    if k == 2:
        base[1::2, :] = 255 - ref[1::2, :]
    elif k == 3:
        base[:, 1::2] = 255 - ref[:, 1::2]
    img = np.clip(base + rs.randint(-60, 61, shape), 0, 255)
    return img.astype(np.uint8), ref.astype(np.uint8)


_PAIRS = {}


def ssim_pairs(shape, win, which=(0, 1, 2, 3)):
    """[(image, reference, ssim_map)] of the chosen input pairs, computed once and shared; nobody writes to them"""
    out = []
    for k in which:
        key = (tuple(shape), win, k)
        if key not in _PAIRS:
            img, ref = ssim_pair(shape, win, k)
            S = M.ssim_map(img, ref, win)
            for a in (img, ref, S):
                a.setflags(write=False)
            _PAIRS[key] = (img, ref, S)
        out.append(_PAIRS[key])
    return out


FINISH_PAIRS = (0, 2)


def dark(shape, rs):
    """dark noise with sparse strong peaks (as in test_gpu_metrics.py)"""
    img = rs.randint(0, 30, shape).astype(np.uint8)
    peaks = rs.rand(*shape) < 0.02
    img[peaks] = rs.randint(80, 256, int(peaks.sum()))
    return img


def dark_set(n_cells, n_angles):
    """3 images against a dark reference: a 30 % corrupted copy, the reference itself, other noise"""
    rs = np.random.RandomState(n_cells + n_angles)
    ref = dark((n_cells, n_angles), rs)
    imgs = np.stack([ref, ref, dark(ref.shape, rs)])
    hit = rs.rand(n_cells, n_angles) < 0.3
    imgs[0][hit] = rs.randint(0, 256, int(hit.sum()))
    return imgs, ref


def hist_inputs(n_cells, n_angles, k=None):
    """[(name, images [n <= 3], reference)] of a histogram case.  "key1": all 0 against all 1 is key 1, the high half of LDS
    word 0, a whole strip in one count (then the reference itself, key 0x0101, and all 2).  "keyFFFF": all 255 against all
    255, the high half of the last word (then 254 and 0: keys 0xFEFF and 0x00FF).  "every_bin", at 65,536 pixels: pixel i is
    (i >> 8, i & 255), so that each bin holds exactly 1."""
    shape = (n_cells, n_angles)
    full = lambda v: np.full(shape, v, np.uint8)
    out = [("dark",) + dark_set(n_cells, n_angles),
           ("key1", np.stack([full(0), full(1), full(2)]), full(1)),
           ("keyFFFF", np.stack([full(255), full(254), full(0)]), full(255))]
    if n_cells * n_angles == 65536:
        i = np.arange(65536)
        out.append(("every_bin", (i >> 8).astype(np.uint8).reshape(1, *shape), (i & 255).astype(np.uint8).reshape(shape)))
    return out


# ---- the cases reach their edges ------------------------------------------------------------------------------------------

def test_constants_are_the_ones_the_cases_were_written_for():
    k = constants()
    assert k["kHistStrip"] % 16 == 0 and k["kHistStrip"] < 1 << 16           # a 16-bit count holds a whole strip
    assert k["kSsimTB"] % k["kSsimTW"] == 0 and k["kSsimTH"] % (k["kSsimTB"] // k["kSsimTW"]) == 0
    assert k["finish_stride"] == k["kSsimTB"] == 256


def test_ssim_cases_sit_at_below_and_above_each_seam():
    k = constants()
    th, tw = k["kSsimTH"], k["kSsimTW"]
    all_cases = cases(k)["ssim"]
    for w in WINDOWS:
        mine = [c for c in all_cases if c.win == w]
        hs, ws = {c.out_h for c in mine}, {c.out_w for c in mine}
        assert {th - 1, th, th + 1} <= hs and 2 * th + 1 in hs, (w, hs)       # the first seam; one row in a third tile
        assert {tw - 1, tw, tw + 1} <= ws and 2 * tw + 1 in ws, (w, ws)
        shapes = {(c.out_h, c.out_w) for c in mine}
        assert {(th, tw), (th + 1, tw + 1), (th - 1, 2 * tw + 1), (2 * th + 1, tw - 1)} <= shapes
        assert len(shapes) == len(mine)
    assert {(c.out_h, c.out_w) for c in all_cases if c.win == 7} >= {(32, 64), (33, 65), (31, 129), (65, 63)}
    assert set(WINDOWS) == {3, 7, 15}
    for c in all_cases:
        n_cells, n_angles = image_shape(c)
        assert c.win <= n_cells <= MAX_CELLS and c.win <= n_angles <= MAX_ANGLES and n_cells * n_angles < MAX_PIXELS
        tiles = -(-c.out_h // th), -(-c.out_w // tw)
        assert ssim_blocks(n_cells, n_angles, c.win, k) == tiles[0] * tiles[1]


def test_finish_cases_have_a_stride_of_partials_one_fewer_and_two_more():
    k = constants()
    fin = cases(k)["finish"]
    assert [c.n_blocks for c in fin] == [k["finish_stride"] - 1, k["finish_stride"], k["finish_stride"] + 2] == [255, 256, 258]
    for c in fin:
        assert ssim_blocks(c.n_cells, c.n_angles, c.win, k) == c.n_blocks, c
        assert c.n_cells <= MAX_CELLS and c.n_angles <= MAX_ANGLES and c.n_cells * c.n_angles < MAX_PIXELS
    assert [(-(-(c.n_cells - 6) // k["kSsimTH"]), -(-(c.n_angles - 6) // k["kSsimTW"])) for c in fin] == [(85, 3), (128, 2), (86, 3)]


def test_histogram_cases_sit_on_the_strip_edges():
    k = constants()
    strip = k["kHistStrip"]
    hist = cases(k)["hist"]
    assert [c.n_px for c in hist] == [strip - 15, strip, strip + 1, strip + 2, strip + 16, 2 * strip, 2 * strip + 3]
    for c in hist:
        assert c.n_cells * c.n_angles == c.n_px, c                            # the shape holds the count its row claims
        assert 1 <= c.n_cells <= MAX_CELLS and 1 <= c.n_angles <= MAX_ANGLES and 3 * c.n_px < 3 * MAX_PIXELS
    last = [c.n_px - (c.n_px - 1) // strip * strip for c in hist]             # pixels of the last strip
    assert last == [strip - 15, strip, 1, 2, 16, strip, 3]
    assert any(0 < n < 16 for n in last) and any(n % 16 and n > 16 for n in last) and 16 in last
    assert hist[0].n_px % 2 == 1                                              # image 1 starts at an odd address
    assert {(c.n_cells, c.n_angles) for c in hist} >= set(ALIGN_SHAPES)
    assert set(ALIGN_OFFSETS) == {(0, 1), (1, 0), (1, 1), (3, 5), (16, 0)}


# ---- the references agree, and the inputs show every position -------------------------------------------------------------

SSIM_CASES = cases()["ssim"]
FINISH_CASES = cases()["finish"]


def every_ssim_input():
    for c in SSIM_CASES:
        yield c.win, image_shape(c), (0, 1, 2, 3)
    for c in FINISH_CASES:
        yield c.win, (c.n_cells, c.n_angles), FINISH_PAIRS


def test_three_references_agree():
    worst = 0.0
    for win, shape, which in every_ssim_input():
        for img, ref, S in ssim_pairs(shape, win, which):
            assert S.shape == (shape[0] - win + 1, shape[1] - win + 1)
            m = float(S.mean(dtype=np.float64))
            d = max(abs(m - M.ssim_integer(img, ref, win)), abs(m - M.ssim(img, ref, win)))
            worst = max(worst, d)
            assert d <= 1e-12, (win, shape, d)
    print("ssim_map against ssim_integer and ssim: at most %.2e" % worst)
    x = np.arange(81, dtype=np.uint8).reshape(9, 9)
    assert np.all(M.ssim_map(x, x, 3) == 1.0) and M.ssim_map(x, x, 9).shape == (1, 1)


@pytest.mark.parametrize("c", SSIM_CASES, ids=case_id)
def test_every_position_and_every_seam_is_visible_in_the_mean(c):
    k = constants()
    S = np.stack([s for _, _, s in ssim_pairs(image_shape(c), c.win)])
    assert S.shape == (4, c.out_h, c.out_w)
    assert np.abs(S).max(axis=0).min() >= VISIBLE
    # the first position of every later tile against its neighbour in the tile before, and the last position against the one before it
    rows = sorted(set(range(k["kSsimTH"], c.out_h, k["kSsimTH"])) | {c.out_h - 1})
    cols = sorted(set(range(k["kSsimTW"], c.out_w, k["kSsimTW"])) | {c.out_w - 1})
    assert rows[0] >= 1 and cols[0] >= 1
    for r in rows:
        assert np.abs(S[:, r] - S[:, r - 1]).max(axis=0).min() >= VISIBLE, ("row", r)
    for q in cols:
        assert np.abs(S[:, :, q] - S[:, :, q - 1]).max(axis=0).min() >= VISIBLE, ("column", q)
    assert S.min() < 0 and S.max() > 0.8                                      # a wide spread, both signs


def test_histogram_inputs_fill_the_bins_they_claim():
    for c in cases()["hist"]:
        inputs = dict((name, (imgs, ref)) for name, imgs, ref in hist_inputs(c.n_cells, c.n_angles))
        assert ("every_bin" in inputs) == (c.n_px == 65536)
        for name, (imgs, ref) in inputs.items():
            assert imgs.dtype == ref.dtype == np.uint8 and imgs.shape[1:] == ref.shape == (c.n_cells, c.n_angles) and len(imgs) <= 3
        H = M.joint_histogram(inputs["key1"][0][0], inputs["key1"][1])
        assert H[0, 1] == c.n_px == H.sum(dtype=np.uint64)
        H = M.joint_histogram(inputs["keyFFFF"][0][0], inputs["keyFFFF"][1])
        assert H[255, 255] == c.n_px == H.sum(dtype=np.uint64)
        for img, key in zip(inputs["key1"][0], (0x0001, 0x0101, 0x0201)):
            assert M.joint_histogram(img, inputs["key1"][1]).ravel()[key] == c.n_px and key & 1
        for img, key in zip(inputs["keyFFFF"][0], (0xFFFF, 0xFEFF, 0x00FF)):
            assert M.joint_histogram(img, inputs["keyFFFF"][1]).ravel()[key] == c.n_px and key & 1
        if "every_bin" in inputs:
            H = M.joint_histogram(inputs["every_bin"][0][0], inputs["every_bin"][1])
            assert np.all(H == 1)
            got = M.info(H)
            assert abs(got["hxy"] - np.log(65536.0)) <= 1e-12 and abs(got["hx"] - np.log(256.0)) <= 1e-12
            assert abs(got["hy"] - np.log(256.0)) <= 1e-12 and abs(got["mi"]) <= 1e-12
        dimgs, dref = inputs["dark"]
        assert np.array_equal(dimgs[1], dref) and not np.array_equal(dimgs[0], dref)
        assert np.count_nonzero(M.joint_histogram(dimgs[0], dref)) > 1000
