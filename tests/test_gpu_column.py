"""k_column on its own: synthetic echo streams through rr_debug_column -- the frame path's launcher and instantiations -- against
orc_column, the oracle's column step (tests/test_column_host.py ties it to orc_simulate, the oracle pins tie that to the reference).

With ambient_noise = 0 the kernel calls no libm and DESIGN.md §4 claims bit equality: every segment's f32 column, u8 column and
last-pass counters are compared exactly.  With noise on, the decay table's expf is the GPU's: the constants of
tests/test_gpu_parity.py over all pixels of the case (test_noise); tests/test_gpu_column_noise.py compares the rest of the noise
path exactly.

A segment's stream is what the kernel stages, in order: the compacted list of passes 0 .. P-2, then the last pass' per-wave
slots -- both records of a wave with record_multi_path, else the even one only; a record with cell < 0 is empty, one with
cell >= n_cells is dropped.  RR_SIG_CHUNK = 1024 staged records make a chunk."""
import sys

import numpy as np
import pytest

from common import GOLDEN, image_diff
from radarays_ros_amd import params
from test_gpu_parity import MEAN_DEV_TOL, U8_MISMATCH_TOL

sys.path.insert(0, GOLDEN)
import gen_oracle_images as gen  # noqa: E402

pytestmark = pytest.mark.gpu

N_ANGLES = 400
CHUNK = 1024
BIG = (2048, 4096)        # (beam samples, max_waves_per_azimuth) -> wave capacity 4096, signal capacity 2048 + 4096
TRI9 = dict(signal_denoising=1, signal_denoising_triangular_width=9, signal_denoising_triangular_mode=0.35)


@pytest.fixture(scope="module")
def ctx(native_lib):
    c = native_lib.Context(0)
    yield c
    c.close()


def config(n_cells, noise=0, scroll=0, **den):
    kw = dict(n_cells=n_cells, n_reflections=2, ambient_noise=noise, scroll_image=scroll, signal_denoising=0)
    kw.update(den)
    return params.RadarModelConfig(**kw)


def denoiser(kind, width, mode):
    """config fields of denoiser `kind` with `width` taps and its peak at tap `mode` (= (int)(fraction * width))"""
    name = {1: "triangular", 2: "gaussian", 3: "mb"}[kind]
    frac = (mode + 0.5) / width
    assert int(frac * width) == mode and 0.0 <= frac < 1.0
    return {"signal_denoising": kind, "signal_denoising_%s_width" % name: width, "signal_denoising_%s_mode" % name: frac}


def strengths(rs, n):
    return np.exp(rs.uniform(np.log(1e-6), np.log(1e3), n)).astype(np.float32)


def echoes(cells, strs):
    from radarays_ros_amd.native import ECHO_DTYPE
    e = np.zeros(len(cells), ECHO_DTYPE)
    e["cell"], e["strength"] = cells, strs
    return e


def with_drops(rs, kept, n_cells):
    """the kept echoes in their order with about a quarter as many dropped ones interleaved at random"""
    n_drop = len(kept) // 4 + 3
    drop = echoes(rs.choice([-1, -7, n_cells, n_cells + 5], n_drop), strengths(rs, n_drop))
    out = np.concatenate([kept, drop])
    is_drop = np.zeros(len(out), bool)
    is_drop[rs.choice(len(out), n_drop, replace=False)] = True
    out[is_drop], out[~is_drop] = drop, kept
    return out


class Seg:
    """one segment: its list, and its last-pass slots (2 records per wave) with the waves' hit bits"""

    def __init__(self, lst=None, slots=None, hit=None):
        self.list = echoes([], []) if lst is None else lst
        self.slots = echoes([], []) if slots is None else slots
        assert len(self.slots) % 2 == 0
        self.waves = len(self.slots) // 2
        self.hit = np.ones(self.waves, np.uint8) if hit is None else np.asarray(hit, np.uint8)


def as_slots(stream):
    """a stream laid into consecutive slots (record_multi_path on): wave j = records 2j, 2j + 1; an odd tail gets an empty slot"""
    s = stream if len(stream) % 2 == 0 else np.concatenate([stream, echoes([-1], [0.0])])
    return s.copy()


def as_even_slots(stream, rs=None):
    """a stream laid into the even slots; the odd ones are empty, or with rs hold echoes nobody may read (record_multi_path off)"""
    s = echoes(np.full(2 * len(stream), -1), np.zeros(2 * len(stream)))
    s[0::2] = stream
    if rs is not None:
        s["cell"][1::2] = rs.randint(0, 64, len(stream))
        s["strength"][1::2] = 1e4
    return s


def run(ctx, oracle, cfg, segs, n_frames, n_loc, az_begin=0, n_passes=2, rmp=True, noise=None, sizing=BIG, exact=True):
    """The segments through rr_debug_column and orc_column.  exact: asserts bit equality and the counters for every segment.
    Returns (gpu f32, gpu u8, ref f32, ref u8), each [n_seg][n_cells]."""
    n_seg = n_frames * n_loc
    assert len(segs) == n_seg
    ctx.set_config(cfg, N_ANGLES, max_waves_per_azimuth=sizing[1])
    ctx.set_beam_samples(np.tile(np.float32([1, 0, 0]), (sizing[0], 1)))
    ctx.set_noise_offsets(np.zeros(N_ANGLES, np.float32) if noise is None else noise)
    ls = max(1, max(len(s.list) for s in segs))
    ws = max(1, max(s.waves for s in segs))
    lst = echoes(np.full(n_seg * ls, -1), np.zeros(n_seg * ls)).reshape(n_seg, ls)
    slots = echoes(np.full(n_seg * 2 * ws, -1), np.zeros(n_seg * 2 * ws)).reshape(n_seg, 2 * ws)
    hit = np.zeros((n_seg, ws), np.uint8)
    for k, s in enumerate(segs):
        lst[k, :len(s.list)] = s.list
        slots[k, :2 * s.waves] = s.slots
        hit[k, :s.waves] = s.hit
    n_beam = segs[0].waves if n_passes == 1 else 7
    gf, g8, gst = ctx.debug_column(n_frames, n_loc, az_begin, n_passes, n_beam, rmp, lst, [len(s.list) for s in segs],
                                   slots, hit, [s.waves for s in segs])
    rows = 1 if noise is None else np.asarray(noise).size // N_ANGLES
    nz = None if noise is None else np.asarray(noise, np.float32).reshape(rows, N_ANGLES)
    rf, r8 = np.zeros_like(gf), np.zeros_like(g8)
    memo = {}
    for k, s in enumerate(segs):
        az = az_begin + k % n_loc
        staged = s.slots if rmp else s.slots[0::2]
        stream = np.concatenate([s.list if n_passes > 1 else s.list[:0], staged])
        off = 0.0 if nz is None else nz[(k // n_loc) % rows, az]
        key = (id(s), float(off), az) if cfg.ambient_noise else id(s)
        if key not in memo:
            memo[key] = oracle.column(cfg, stream["cell"], stream["strength"], off, (cfg.scroll_image + az) % N_ANGLES, N_ANGLES)
        rf[k], r8[k] = memo[key]
        if exact:
            assert np.array_equal(gf[k], rf[k], equal_nan=True), ("f32", k, np.flatnonzero(gf[k].view(np.uint32) != rf[k].view(np.uint32))[:8])
            assert np.array_equal(g8[k], r8[k]), ("u8", k, np.flatnonzero(g8[k] != r8[k])[:8])
        hits = int(s.hit.sum())                  # (the hit bit lives in the even slot: staged either way)
        assert tuple(gst[k]) == (s.waves, hits, int((staged["cell"] >= 0).sum())), ("wave_passes, hits, signals", k, tuple(gst[k]))
    return gf, g8, rf, r8


def three_forms(stream):
    """the same stream as a list with no waves, as slots alone, and as a list that ends mid-chunk with the slots going on in
    the same chunk"""
    cut = len(stream) // 2 if len(stream) <= CHUNK else len(stream) - CHUNK // 3
    return [Seg(stream), Seg(None, as_slots(stream)), Seg(stream[:cut], as_slots(stream[cut:]))]


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drops", [False, True], ids=["kept", "with_drops"])
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 2500])
@pytest.mark.parametrize("den", [{}, TRI9], ids=["fmax", "tri9"])
def test_chunk_edges(ctx, oracle, den, count, drops):
    """`count` kept echoes per segment -- around the wave (64), the chunk (1024) and two chunks; with drops interleaved the
    staged count differs from the kept one and a chunk of 1024 staged records keeps fewer.  None of the staged counts with
    drops is a multiple of 256 or 512."""
    n_cells = 200
    rs = np.random.RandomState(1000 + count + (5000 if drops else 0))
    stream = echoes(rs.randint(0, n_cells, count), strengths(rs, count))
    if drops:
        stream = with_drops(rs, stream, n_cells)
        assert len(stream) % 256 != 0
    segs = three_forms(stream)
    gf, g8, rf, r8 = run(ctx, oracle, config(n_cells, **den), segs, 1, 3)
    assert np.array_equal(gf[0], gf[1], equal_nan=True) and np.array_equal(gf[0], gf[2], equal_nan=True)


@pytest.mark.parametrize("n_cells", [1, 2, 63, 64, 65, 130, 3424, 4096, 4097, 8192])
@pytest.mark.parametrize("den", [{}, TRI9, denoiser(1, 65, 32)], ids=["fmax", "tri9", "tri65"])
def test_tile_and_column_edges(ctx, oracle, den, n_cells):
    """Echoes on the first and last bins of the column and of its 64-bin tiles, and for the two widest columns on the bins where
    the tile mask changes words (tile 63 | 64 = bin 4095 | 4096).  Bin 0 stays unwritten under a window that covers it."""
    rs = np.random.RandomState(n_cells)
    special = [0, 1, 62, 63, 64, n_cells - 2, n_cells - 1] + ([4095, 4096, 4097] if n_cells > 4096 else [])
    special = np.array([c for c in special if 0 <= c], np.int64)          # (4097 in a column of 4097: dropped)
    alone = [Seg(echoes([c], [2.5])) for c in special]                                   # one echo per column
    once = Seg(echoes(special, strengths(rs, len(special))))                              # all of them, in order
    mixed = np.concatenate([np.repeat(special, 3), rs.randint(0, n_cells, 300)])
    mixed = Seg(echoes(rs.permutation(mixed), strengths(rs, len(mixed))))
    segs = alone + [once, mixed]
    gf, g8, rf, r8 = run(ctx, oracle, config(n_cells, **den), segs, 1, len(segs))
    if den:          # (a column whose every echo was dropped, or fell on bin 0 alone, is empty: NaN)
        assert not (np.nan_to_num(gf[:, 0]) != 0).any() and not g8[:, 0].any()
        if n_cells > 1:
            assert gf[-2, 1] > 0
    else:
        assert gf[0, 0] > 0            # the fmaxf path does write bin 0 (RadarCPU.cpp:439)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("width", [1, 2, 63, 64, 65, 256])
@pytest.mark.parametrize("kind", [1, 2, 3])
def test_denoiser_windows(ctx, oracle, kind, width, where):
    """Every denoiser kind at widths around the tile size and at the largest, its peak on the first, a middle and the last tap
    (mode 0 gives the reference's 0/0 weights: NaN bins, compared as such).  Columns of 300 bins clip the windows of the echoes near
    either end; a column of 40 bins is narrower than the wide windows, which are clipped at both ends."""
    mode = {"first": 0, "middle": width // 2, "last": width - 1}[where]
    for n_cells in (300, 40):
        rs = np.random.RandomState(kind * 1000 + width)
        edge = [0, 1, 2, max(mode - 1, 0), mode, mode + 1, n_cells - 1, n_cells - 2, max(n_cells - width + mode, 0), n_cells // 2]
        cells = np.concatenate([np.array(edge) % n_cells, rs.randint(0, n_cells, 120)])
        segs = [Seg(echoes([c], [3.0])) for c in (0, mode % n_cells, n_cells - 1)]
        segs.append(Seg(echoes(rs.permutation(cells), strengths(rs, len(cells)))))
        run(ctx, oracle, config(n_cells, **denoiser(kind, width, mode)), segs, 1, len(segs))


def test_fmax_path_with_echoes_on_the_same_cell(ctx, oracle):
    """signal_denoising = 0: a bin is the largest echo that fell on it (RadarCPU.cpp:439), within a 64-echo batch and across
    batches and chunks."""
    rs = np.random.RandomState(3)
    n_cells = 70
    few = echoes([5, 5, 5, 69, 5, 0, 0, 69], [1.0, 3.0, 2.0, 0.5, 3.0, 1e-6, 2e-6, 0.25])
    many = echoes(rs.choice([0, 5, 63, 64, 69], 1300), strengths(rs, 1300))
    segs = [Seg(few), Seg(many), Seg(None, as_slots(many)), Seg(many[:700], as_slots(many[700:]))]
    gf, _, _, _ = run(ctx, oracle, config(n_cells), segs, 1, 4)
    assert np.array_equal(gf[1], gf[2]) and np.array_equal(gf[1], gf[3])


ODD = {"negative": -40.0, "minus_zero": -0.0, "nan": np.nan, "inf": np.inf}


@pytest.mark.parametrize("chunk", [0, 1], ids=["in_first_chunk", "in_second_chunk"])
@pytest.mark.parametrize("odd", sorted(ODD))
@pytest.mark.parametrize("den", [{}, TRI9, denoiser(3, 64, 25)], ids=["fmax", "tri9", "mb64"])
def test_chunk_that_is_not_simple(ctx, oracle, den, odd, chunk):
    """1500 ordinary echoes and one that is negative, -0.0, NaN or +inf.  In the first chunk: that chunk replays in the general
    form, the second in the simple one; in the second chunk: the other way round."""
    n_cells = 150
    rs = np.random.RandomState(77)
    cells = rs.randint(0, n_cells, 1500)
    cells[:8] = [0, 1, 2, 3, 149, 148, 64, 63]
    strs = strengths(rs, 1500)
    at = 500 if chunk == 0 else 1300
    cells[at], strs[at] = 70, ODD[odd]
    cells[at - 1], strs[at - 1] = 70, 900.0          # the bin of the odd echo has risen before it falls
    stream = echoes(cells, strs)
    run(ctx, oracle, config(n_cells, **den), three_forms(stream), 1, 3)


@pytest.mark.parametrize("den", [{}, TRI9], ids=["fmax", "tri9"])
def test_running_maximum_and_degenerate_columns(ctx, oracle, den):
    """max_val is the largest value any bin ever held (RadarCPU.cpp:428-431), not the largest final one; a column of negative
    echoes and an empty column have max_val = 0: x / 0 scales them to NaN (0 * inf) or -inf, mono8 0."""
    n_cells = 100
    rise_fall = echoes([40, 10, 40, 10], [10.0, 1.0, -8.0, 1.5])      # bin 40: 10, then 2; bin 10 ends as the largest final bin
    negative = echoes([3, 50, 50, 99], [-1.0, -2.0, -0.5, -1e-3])
    empty = echoes([], [])
    all_dropped = echoes([-1, n_cells, n_cells + 5], [1.0, 2.0, 3.0])
    segs = [Seg(rise_fall), Seg(negative), Seg(empty), Seg(all_dropped), Seg(None, as_slots(rise_fall)), Seg(None, as_slots(negative))]
    cfg = config(n_cells, **den)
    gf, g8, rf, r8 = run(ctx, oracle, cfg, segs, 1, len(segs))
    scale = np.float32(cfg.signal_max / np.float64(np.float32(10.0)))
    if den:
        assert gf[0, 40] == np.float32(np.float32(10.0 - 8.0) * np.float32(cfg.energy_max)) * scale       # w[mode] = 1
        assert gf[0].max() < 0.5 * cfg.signal_max * cfg.energy_max       # scaled by the running maximum 10, not by a final bin
        assert np.isneginf(gf[1]).any()
    assert np.array_equal(gf[0], gf[4]) and np.array_equal(gf[1], gf[5], equal_nan=True)
    assert not (gf[1] > 0).any() and np.isnan(gf[1]).any() and not g8[1].any()
    assert np.isnan(gf[2]).all() and np.isnan(gf[3]).all() and not g8[2].any() and not g8[3].any()


@pytest.mark.parametrize("noise", [1, 2])
def test_empty_columns_with_noise(ctx, oracle, noise):
    """x / 0 with the noise on, as test_degenerate_inputs states for frames: a NaN f32 column and a mono8 column of zeros."""
    segs = [Seg(echoes([], [])), Seg(echoes([-1, 64], [1.0, 1.0])), Seg(None, as_slots(echoes([-1, -1, -1], [0, 0, 0])))]
    rnd = (np.random.RandomState(5).uniform(0, 1, N_ANGLES) * 1000.0).astype(np.float32)
    gf, g8, rf, r8 = run(ctx, oracle, config(64, noise=noise, **TRI9), segs, 1, 3, az_begin=11, noise=rnd)
    assert np.isnan(gf).all() and not g8.any()


# ---------------------------------------------------------------------------------------------------------------------------
def test_stream_forms(ctx, oracle):
    """The list alone with a last pass of no waves; the slots alone (one pass: every segment stages n_beam waves); both, the
    list ending mid-chunk."""
    n_cells = 260
    rs = np.random.RandomState(11)
    a = with_drops(rs, echoes(rs.randint(0, n_cells, 1400), strengths(rs, 1400)), n_cells)
    b = with_drops(rs, echoes(rs.randint(0, n_cells, 300), strengths(rs, 300)), n_cells)
    cfg = config(n_cells, **TRI9)
    g_list, _, _, _ = run(ctx, oracle, cfg, [Seg(a), Seg(b)], 2, 1)
    both = echoes(np.full(2 * len(a), -1), np.zeros(2 * len(a))).reshape(2, len(a))
    both[0], both[1, :len(b)] = a, b
    f, u, st = ctx.debug_column(2, 1, 0, 2, 0, True, echoes=both, echo_count=[len(a), len(b)])          # no slot arrays at all
    assert np.array_equal(f, g_list, equal_nan=True) and not st.any()
    waves = (len(a) + 1) // 2

    def pad(s):              # the stream in consecutive slots of `waves` waves, the rest empty
        out = echoes(np.full(2 * waves, -1), np.zeros(2 * waves))
        out[:len(s)] = s
        return out
    g_slots, _, _, _ = run(ctx, oracle, cfg, [Seg(a[:5], pad(a)), Seg(None, pad(b))], 1, 2, n_passes=1)       # (one pass: the list is not read)
    assert np.array_equal(g_slots, g_list, equal_nan=True)
    g_both, _, _, _ = run(ctx, oracle, cfg, [Seg(a[:700], as_slots(a[700:])), Seg(b[:1], as_slots(b[1:]))], 1, 2)
    assert np.array_equal(g_both, g_list, equal_nan=True)


def test_record_multi_path_on_and_off(ctx, oracle):
    """On: echoes in the odd slots, an empty even slot beside a full odd one, a hit bit on a wave without an echo, waves that
    missed.  Off: only the even slots are staged (stride 2) -- whatever the odd ones hold -- and give the columns of the same
    even slots with it on and the odd ones empty; the counters see the even slots only."""
    n_cells = 180
    rs = np.random.RandomState(21)
    cfg = config(n_cells, **TRI9)
    for waves in (5, 700, 1500):               # (1500 waves: 3000 slots = three chunks with it on, two with it off)
        s = echoes(rs.randint(0, n_cells, 2 * waves), strengths(rs, 2 * waves))
        s["cell"][rs.uniform(size=2 * waves) < 0.4] = -1
        s["cell"][0], s["cell"][1] = -1, 7                  # an empty even slot beside a full odd one
        s["cell"][2], s["cell"][3] = -1, -1                 # a wave that hit (bit set below) and left no echo
        hit = (rs.uniform(size=waves) < 0.7).astype(np.uint8)
        hit[0], hit[1] = 0, 1
        lst = echoes(rs.randint(0, n_cells, 100), strengths(rs, 100))
        on = run(ctx, oracle, cfg, [Seg(lst, s, hit), Seg(None, s, hit)], 1, 2, rmp=True)
        even = as_even_slots(s[0::2])
        garbage = as_even_slots(s[0::2], rs)
        off = run(ctx, oracle, cfg, [Seg(lst, garbage, hit), Seg(None, garbage, hit)], 1, 2, rmp=False)
        on_even = run(ctx, oracle, cfg, [Seg(lst, even, hit), Seg(None, even, hit)], 1, 2, rmp=True)
        assert np.array_equal(off[0], on_even[0], equal_nan=True) and np.array_equal(off[1], on_even[1])
        assert not np.array_equal(on[0], off[0], equal_nan=True)


def test_both_instantiations(ctx, oracle):
    """launch_column runs k_column<256> for a launch of at least 1024 segments and k_column<512> below: the same 8 streams tiled over
    1024 + 16 segments and over 16, every segment equal to the reference and to its twin in the other launch."""
    n_cells = 130
    rs = np.random.RandomState(31)
    ordinary = lambda n: echoes(rs.randint(0, n_cells, n), strengths(rs, n))      # noqa: E731
    neg = ordinary(1400)
    neg["strength"][1200] = -3.0
    streams = [Seg(ordinary(0)), Seg(ordinary(1)), Seg(with_drops(rs, ordinary(300), n_cells)), Seg(ordinary(1025)),
               Seg(ordinary(1000), as_slots(with_drops(rs, ordinary(600), n_cells))), Seg(None, as_slots(ordinary(2047))),
               Seg(neg), Seg(echoes([0, 1, 63, 64, 65, 127, 128, 129], strengths(rs, 8)))]
    cfg = config(n_cells, **TRI9)
    sizing = (512, 1024)              # wave capacity 1024, signal capacity 1536: 1040 segments stay small
    wide = run(ctx, oracle, cfg, [streams[k % 8] for k in range(1040)], 4, 260, sizing=sizing)
    narrow = run(ctx, oracle, cfg, [streams[k % 8] for k in range(16)], 1, 16, sizing=sizing)
    for k in range(1040):
        assert np.array_equal(wide[0][k], narrow[0][k % 8], equal_nan=True) and np.array_equal(wide[1][k], narrow[1][k % 8]), k


@pytest.mark.parametrize("rows", ["one_row", "row_per_frame"])
@pytest.mark.parametrize("den", [{}, TRI9], ids=["fmax", "tri9"])
@pytest.mark.parametrize("noise", [1, 2], ids=["uniform", "perlin"])
def test_noise(ctx, oracle, noise, den, rows):
    """Ambient noise 1 and 2 on 64 segments x 3424 bins, every column with its own offset, one row of offsets or one per frame,
    az_begin > 0, n_loc < n_angles and a scroll, so that the azimuth, the image column and the noise row are different numbers.
    Columns of three kinds: echoes in one 64-bin tile only (every other wave takes the "all 64 bins empty" amplitude), echoes in
    every tile, and tiles whose only non-zero bin is their last.  This is the statistical check over the one term that is not
    exact, the decay table's expf (the GPU's libm), at the presets' energies and the full column width: the tolerances of
    tests/test_gpu_parity.py over all pixels.  The exact checks are next door, tests/test_gpu_column_noise.py: everything but
    that term bit for bit, and expf bounded per pixel."""
    n_cells, n_frames, n_loc, az_begin = 3424, 4, 16, 100
    rs = np.random.RandomState(41 + noise)
    first_nonzero = 2 if den else 0          # tri9, mode 3: tap 0 weighs 0, tap 1 is the window's first non-zero bin
    segs = []
    for k in range(n_frames * n_loc):
        kind = k % 3
        if kind == 0:
            t = rs.randint(0, n_cells // 64)
            cells = rs.randint(64 * t + 8, 64 * t + 56, 40)
        elif kind == 1:
            cells = np.concatenate([np.arange(0, n_cells, 64) + rs.randint(0, 64), rs.randint(0, n_cells, 200)])
            cells = cells[cells < n_cells]
        else:
            cells = 64 * rs.choice(n_cells // 64 - 1, 6, replace=False) + 63 + first_nonzero
        segs.append(Seg(echoes(cells, strengths(rs, len(cells)))))
    n_rows = 1 if rows == "one_row" else n_frames
    rnd = (rs.uniform(0, 1, (n_rows, N_ANGLES)) * 1000.0).astype(np.float32)
    cfg = config(n_cells, noise=noise, scroll=37, **den)
    gf, g8, rf, r8 = run(ctx, oracle, cfg, segs, n_frames, n_loc, az_begin=az_begin, noise=rnd, exact=False)
    assert np.isfinite(rf).all()
    d = image_diff(gf, rf, g8, r8)
    msg = "u8 mismatch share %.3g (allowed %.3g = %d of %d pixels), mean deviation %.3g (allowed %.3g), u8 max %d" % (
        d["u8_mismatch_frac"], U8_MISMATCH_TOL, int(U8_MISMATCH_TOL * g8.size), g8.size, d["mean_dev"], MEAN_DEV_TOL, d["u8_max"])
    print(msg)
    assert d["mean_dev"] <= MEAN_DEV_TOL, msg
    assert d["u8_max"] <= 1 and d["u8_mismatch_frac"] <= U8_MISMATCH_TOL, msg


def test_one_realistic_stream(ctx, oracle):
    """The echo streams a real sweep logged (gen.case_multibounce, tests/test_column_host.py) through rr_debug_column: the
    synthetic entry on a frame's own data, half of every stream in the list and half in the slots."""
    from test_column_host import logged_sweep
    cfg, rnd, az, u8, f32, log = logged_sweep(oracle, gen.case_multibounce)
    busiest = np.argsort(-log["counts"].astype(np.int64), kind="stable")[:32]
    assert log["counts"][busiest].min() > 0
    order = np.sort(busiest)
    segs = []
    for a in order:
        s = echoes(log["cells"][a, :log["counts"][a]], log["strengths"][a, :log["counts"][a]])
        segs.append(Seg(s[:len(s) // 2], as_slots(s[len(s) // 2:])))
    ctx.set_config(cfg, N_ANGLES)
    nb = 64                              # the case's beam: wave capacity 512, signal capacity 960 over its 4 passes
    ls, ws = max(len(s.list) for s in segs), max(s.waves for s in segs)
    lst = echoes(np.full(32 * ls, -1), np.zeros(32 * ls)).reshape(32, ls)
    slots = echoes(np.full(32 * 2 * ws, -1), np.zeros(32 * 2 * ws)).reshape(32, 2 * ws)
    for k, s in enumerate(segs):
        lst[k, :len(s.list)], slots[k, :2 * s.waves] = s.list, s.slots
    ctx.set_beam_samples(np.tile(np.float32([1, 0, 0]), (nb, 1)))
    gf, g8, st = ctx.debug_column(1, 32, 0, cfg.n_reflections, nb, True, lst, [len(s.list) for s in segs], slots,
                                  np.ones((32, ws), np.uint8), [s.waves for s in segs])
    for k, a in enumerate(order):
        col = (cfg.scroll_image + int(a)) % N_ANGLES
        assert np.array_equal(gf[k], f32[:, col], equal_nan=True) and np.array_equal(g8[k], u8[:, col]), int(a)
        rf, r8 = oracle.column(cfg, log["cells"][a, :log["counts"][a]], log["strengths"][a, :log["counts"][a]], 0.0, col)
        assert np.array_equal(gf[k], rf, equal_nan=True) and np.array_equal(g8[k], r8)


def test_refusals(native_lib):
    """What the lane's buffers cannot hold is refused with -3 and a message, and nothing is written."""
    c = native_lib.Context(0)
    with pytest.raises(native_lib.RRError, match="rr_set_config"):
        c.debug_column(1, 1)
    cfg = config(64)
    c.set_config(cfg, N_ANGLES, max_waves_per_azimuth=16)
    c.set_beam_samples(np.tile(np.float32([1, 0, 0]), (8, 1)))          # wave capacity 16, signal capacity 8 + 16
    e = echoes(np.zeros(40), np.ones(40))
    ok = dict(n_frames=1, n_loc=1, az_begin=0, n_passes=2, n_beam=8, record_multi_path=True, echoes=e[:24], echo_count=[24], slots=e[:32],
              slot_hit=np.ones(16), slot_count=[16])
    f, u, st = c.debug_column(**ok)
    assert tuple(st[0]) == (16, 16, 32) and u[0, 0] == 60
    bad = [(dict(n_frames=0), "n_frames"), (dict(n_frames=65), "n_frames"), (dict(n_loc=0), "azimuth block"),
           (dict(az_begin=N_ANGLES), "azimuth block"), (dict(az_begin=-1), "azimuth block"), (dict(n_loc=N_ANGLES + 1), "azimuth block"),
           (dict(n_passes=0), "n_passes"), (dict(n_passes=3), "n_passes"), (dict(n_beam=-1), "n_beam"), (dict(n_beam=17), "wave capacity"),
           (dict(echoes=e[:25], echo_count=[25]), "signal capacity"), (dict(echo_count=[25]), "list count"),
           (dict(slots=e[:34], slot_hit=np.ones(17), slot_count=[17]), "wave capacity"), (dict(slot_count=[17]), "slot count"),
           (dict(n_passes=1, n_beam=16, slots=e[:30], slot_hit=np.ones(15)), "n_beam waves"), (dict(slot_count=None), "null stream")]
    for change, text in bad:
        kw = dict(ok)
        kw.update(change)
        n_seg = max(kw["n_frames"] * kw["n_loc"], 1)
        for k in ("echoes", "slots", "slot_hit"):
            kw[k] = np.tile(kw[k], (n_seg, 1))
        for k in ("echo_count", "slot_count"):
            kw[k] = None if kw[k] is None else kw[k] * n_seg
        if kw["n_frames"] * kw["n_loc"] == 0:          # (the binding cannot shape arrays for no segment)
            L = native_lib.lib()
            out = np.full(64, 7, np.uint8)
            rc = L.rr_debug_column(c._h, kw["n_frames"], kw["n_loc"], 0, 2, 8, 1, None, None, 0, None, None, None, 0, None, out.ctypes.data, None)
            assert rc == -3 and (out == 7).all() and text in L.rr_last_error(c._h).decode(), change
            continue
        with pytest.raises(native_lib.RRError, match=text + ".*rc=-3") as ei:
            c.debug_column(**kw)
        assert "rr_debug_column" in str(ei.value), change
    # nothing written by a refused call
    L = native_lib.lib()
    out8, outf, outs = np.full(64, 7, np.uint8), np.full(64, 7, np.float32), np.full(3, 7, np.uint32)
    cnt = np.array([25], np.uint32)
    rc = L.rr_debug_column(c._h, 1, 1, 0, 2, 8, 1, e.ctypes.data, cnt.ctypes.data, 24, None, None, None, 0, outf.ctypes.data, out8.ctypes.data,
                           outs.ctypes.data)
    assert rc == -3 and (out8 == 7).all() and (outf == 7).all() and (outs == 7).all()
    f2, u2, st2 = c.debug_column(**ok)                    # ... and the context is as good as before
    assert np.array_equal(f2, f) and np.array_equal(u2, u) and np.array_equal(st2, st)
    c.close()
