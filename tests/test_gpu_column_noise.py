"""k_column's ambient-noise path against orc_column, bit for bit.  tests/test_gpu_column.py holds the kernel exactly with the
noise off and statistically with it on (test_noise: the decay table's expf is the GPU's libm).  Here the decay term is taken out
of the comparison -- ambient_noise_energy_max == ambient_noise_energy_min makes it 0 * decay[i] + e_min, energy_loss = 0 makes
it expf(-0.0f) on both sides -- and everything else the kernel restructures is compared exactly: the per-column Perlin tables
(lattice wrap, y = 0 rows, negative and huge offsets), the uniform hash and its seed conversion, the precomputed amplitude of an
empty wave, the two squarings for pow(x, 4), the noise row of a frame, the reuse of the replay region's LDS, and both
instantiations.  expf itself is then bounded pixel by pixel in ulps (test_expf_is_within_its_documented_error).

The inputs come from tests/column_noise_cases.py; tests/test_column_noise_host.py proves on the CPU that on them the fourth power
narrows to the same f32 whichever way it is formed, so no assertion here carries an excuse list."""
import numpy as np
import pytest

import column_noise_cases as cases
from test_gpu_column import N_ANGLES, Seg, config, echoes, run

pytestmark = pytest.mark.gpu

E_FLAT = 0.3


@pytest.fixture(scope="module")
def ctx(native_lib):
    c = native_lib.Context(0)
    yield c
    c.close()


def flat(n_cells, noise, e, scroll=0, **den):
    """a config whose decay term is 0 * decay[i] + e"""
    return config(n_cells, noise=noise, scroll=scroll, ambient_noise_energy_max=e, ambient_noise_energy_min=e, **den)


def drive(ctx, oracle, cfg, pool, layout, off, one_row=False, **kw):
    """The pool's columns over one block of azimuths, exactly.  A row of offsets per entry of `off`, each row one offset, and one
    frame more than rows (the last frame wraps to row 0); or one row whose offset changes with the azimuth, and two frames.  The
    column of segment (frame f, azimuth a) is pool[(a + f * (n_loc + 1)) % len(pool)]: it changes with either."""
    az_begin, scroll, n_loc = layout
    assert cfg.scroll_image == scroll
    if one_row:
        rnd, n_frames = off[np.arange(N_ANGLES) % len(off)], 2
    else:
        rnd, n_frames = np.repeat(off, N_ANGLES).reshape(len(off), N_ANGLES), len(off) + 1
    segs = [pool[(k + k // n_loc) % len(pool)] for k in range(n_frames * n_loc)]
    return run(ctx, oracle, cfg, segs, n_frames, n_loc, az_begin=az_begin, noise=rnd, **kw)


def drive_kinds(ctx, oracle, make_cfg, n_cells, noise, layouts, with_one_row=True):
    """every kind of column_noise_cases.column_kinds under its denoiser, over the layouts"""
    kinds = cases.column_kinds(n_cells, seed=n_cells)
    off = cases.offsets_of(noise)
    for den in ({}, cases.TRI9):
        pool = [s for name, s in kinds.items() if cases.den_of(name) == den]
        for lay in (layouts if not den else layouts[1:3]):
            drive(ctx, oracle, make_cfg(scroll=lay[1], **den), pool, lay, off)
        if with_one_row:
            drive(ctx, oracle, make_cfg(scroll=layouts[1][1], **den), pool, layouts[1], off, one_row=True)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cells", [1, 63, 64, 65, 200, 513])
@pytest.mark.parametrize("e", [0.0, E_FLAT], ids=["e0", "e0.3"])
@pytest.mark.parametrize("noise", [1, 2], ids=["uniform", "perlin"])
def test_exact_noise_without_the_decay_term(ctx, oracle, noise, e, n_cells):
    """Step 1: e_max == e_min, at 0 and at 0.3.  Eight kinds of column x every offset x the image columns 0, 5, 20, 100, 399 and
    their neighbours, a row of offsets per frame with one frame more than rows, and one row for all frames: every f32 and u8
    pixel of every segment equals the oracle's."""
    drive_kinds(ctx, oracle, lambda **kw: flat(n_cells, noise, e, **kw), n_cells, noise, cases.LAYOUTS)


@pytest.mark.parametrize("noise", [1, 2], ids=["uniform", "perlin"])
def test_exact_noise_in_the_widest_column(ctx, oracle, noise):
    """8192 bins, the most rr_set_config takes, two segments a denoiser: the four Perlin tables lie in the replay region's LDS
    beside a slice of 32 KB, and neither may reach into the other."""
    n_cells, lay = 8192, (15, 5, 2)
    kinds = cases.column_kinds(n_cells, seed=n_cells)
    rnd = np.zeros(N_ANGLES, np.float32)
    rnd[15:17] = [255.96875, -256.25]
    for den, names in (({}, ["every_tile", "one_tile"]), (cases.TRI9, ["falls_to_zero_beside_echoes", "falls_to_zero"])):
        run(ctx, oracle, flat(n_cells, noise, E_FLAT, scroll=lay[1], **den), [kinds[n] for n in names], 1, 2, az_begin=lay[0], noise=rnd)
    cfg = config(n_cells, noise=noise, scroll=lay[1], ambient_noise_energy_loss=0.0)                  # step 2's config
    run(ctx, oracle, cfg, [kinds["every_tile"], kinds["last_bin"]], 1, 2, az_begin=lay[0], noise=rnd)


@pytest.mark.parametrize("noise", [1, 2], ids=["uniform", "perlin"])
def test_exact_noise_in_both_instantiations(ctx, oracle, noise):
    """3 frames x 342 azimuths of 64 bins are 1026 segments: k_column<256>, the variant a frame batch runs.  The same columns in
    launches of 684 and 342 segments are k_column<512>.  Every segment equals the oracle's column, and segment k of the wide
    launch its twin of the narrow ones."""
    n_cells, n_loc, az_begin, scroll = 64, 342, 58, 347               # image columns 5 .. 346
    kinds = cases.column_kinds(n_cells, seed=n_cells)
    pool = [s for name, s in kinds.items() if not cases.den_of(name)]
    off = cases.offsets_of(noise)
    rs = np.random.RandomState(7)
    rnd = off[rs.randint(0, len(off), (3, N_ANGLES))]
    segs = [pool[(k + k // n_loc) % len(pool)] for k in range(3 * n_loc)]
    cfg = flat(n_cells, noise, E_FLAT, scroll=scroll)
    kw = dict(az_begin=az_begin, sizing=(512, 1024))
    wide = run(ctx, oracle, cfg, segs, 3, n_loc, noise=rnd, **kw)
    two = run(ctx, oracle, cfg, segs[:2 * n_loc], 2, n_loc, noise=rnd, **kw)          # rows 0, 1 of three: frame f reads row f
    last = run(ctx, oracle, cfg, segs[2 * n_loc:], 1, n_loc, noise=rnd[2], **kw)
    narrow_f, narrow_8 = np.concatenate([two[0], last[0]]), np.concatenate([two[1], last[1]])
    for k in range(3 * n_loc):
        assert np.array_equal(wide[0][k], narrow_f[k], equal_nan=True) and np.array_equal(wide[1][k], narrow_8[k]), k


@pytest.mark.parametrize("n_cells", [65, 513])
@pytest.mark.parametrize("noise", [1, 2], ids=["uniform", "perlin"])
def test_exact_noise_with_no_energy_loss(ctx, oracle, noise, n_cells):
    """Step 2: e_max != e_min (0.5, 0.1) and ambient_noise_energy_loss = 0.  The decay table holds expf(-0.0f) in every bin, so
    (e_max - e_min) * decay[i] + e_min and the table's indexing are compared exactly."""
    drive_kinds(ctx, oracle, lambda **kw: config(n_cells, noise=noise, ambient_noise_energy_loss=0.0, **kw), n_cells, noise,
                cases.LAYOUTS[:3], with_one_row=False)


@pytest.mark.parametrize("key", sorted(cases.RANDOM_SEEDS), ids=lambda k: "%s-%d" % k)
@pytest.mark.parametrize("noise", [1, 2], ids=["uniform", "perlin"])
def test_exact_noise_on_arbitrary_strengths(ctx, oracle, noise, key):
    """Step 3: log-uniform strengths, no denoiser, tri9 and mb64.  The seeds are those of column_noise_cases.RANDOM_SEEDS, for
    which tests/test_column_noise_host.py proves that pow(x, 4.0) and two squarings narrow alike in every bin: bit equality,
    with nothing excused."""
    den, n_cells = key
    pool = cases.random_columns(cases.RANDOM_SEEDS[key], n_cells)
    for lay in cases.LAYOUTS[:3]:
        drive(ctx, oracle, flat(n_cells, noise, E_FLAT, scroll=lay[1], **cases.DENOISERS[den]), pool, lay, cases.offsets_of(noise))


# ---------------------------------------------------------------------------------------------------------------------------
EXPF_ULPS = 4


@pytest.mark.parametrize("n_cells", [200, 8192])
@pytest.mark.parametrize("loss", [0.05, 0.3])
@pytest.mark.parametrize("noise", [1, 2], ids=["uniform", "perlin"])
def test_expf_is_within_its_documented_error(ctx, oracle, noise, loss, n_cells):
    """Step 4: the GPU's expf bounded per pixel.  ambient_noise_at_signal_0 = _1 = 0 makes the noise amplitude 0, one echo of 2.0
    in bin 0 (no denoiser) makes max_val = 2: bin i is |(E1 - E0) * decay[i] + E0| * final_scale (+ the signal in bin 0) with
    E1 = 2 * 0.5 > E0 = 2 * 0.1 > 0, at the presets' energy_loss 0.05 and at 0.3.  The reference is that expression in numpy
    f32 with decay[i] = exp in f64, rounded to f32 -- the correctly rounded value.

    The bound, EXPF_ULPS = 4 spacings of the reference pixel:  the HIP math API documentation gives expf a maximum error of
    1 ulp, so the GPU's decay[i] is the reference's or a neighbouring f32: a relative change of at most 2^-23.  The multiply by
    E1 - E0 keeps the relative change; a spacing is at least 2^-24 of its number, so the exact products lie at most 2 spacings
    apart, and rounding is monotonic: 2 after it.  Adding E0 > 0 to a positive product only makes the number and its spacing
    larger: still 2.  The final scale is a multiply again, which can double the count: 4.  (Bin 0 adds its signal first, which
    like E0 only shrinks the count.  Where exp falls below the normal range, at energy_loss 0.3 beyond bin 6640, the product
    vanishes against E0 and the pixel is the same float whatever the GPU returns there.)  The distances seen are printed."""
    cfg = config(n_cells, noise=noise, ambient_noise_at_signal_0=0.0, ambient_noise_at_signal_1=0.0, ambient_noise_energy_loss=loss)
    assert cfg.ambient_noise_energy_max == 0.5 and cfg.ambient_noise_energy_min == 0.1 and cfg.energy_max == 0.5
    rnd = np.full(N_ANGLES, 255.96875, np.float32)
    gf, g8, rf, r8 = run(ctx, oracle, cfg, [Seg(echoes([0], [2.0]))] * 2, 1, 2, az_begin=19, noise=rnd, exact=False)
    f32 = np.float32
    max_val = f32(2.0)
    x = ((np.arange(n_cells).astype(f32).astype(np.float64) + 0.5) * cfg.resolution).astype(f32)
    arg = -f32(loss) * x
    assert arg.dtype == f32
    decay = np.exp(arg.astype(np.float64)).astype(f32)
    e1, e0 = f32(np.float64(max_val) * 0.5), f32(np.float64(max_val) * 0.1)
    y = np.abs((f32(0.0) + (e1 - e0) * decay) + e0)
    signal = np.zeros(n_cells, f32)
    signal[0] = max_val * f32(cfg.energy_max)
    want = (signal + y) * f32(cfg.signal_max / np.float64(max_val))
    assert want.dtype == f32 and np.isfinite(want).all() and (want > 0).all()
    ulps = np.abs(gf.astype(np.float64) - want.astype(np.float64)) / np.spacing(want).astype(np.float64)
    worst = float(ulps.max())
    print("expf: largest distance %.1f spacings at bin %d (allowed %d); %d of %d pixels differ; vs the oracle's libm %.1f" % (
        worst, int(ulps.max(axis=0).argmax()), EXPF_ULPS, int((ulps > 0).sum()), ulps.size,
        float((np.abs(gf.astype(np.float64) - rf.astype(np.float64)) / np.spacing(np.abs(rf)).astype(np.float64)).max())))
    assert worst <= EXPF_ULPS
    assert np.array_equal(gf[0], gf[1])


def test_expf_of_minus_zero_is_one(ctx, oracle):
    """what step 2 rests on, seen directly: with energy_loss = 0 and a zero amplitude every empty bin is (E1 - E0) * 1 + E0"""
    cfg = config(200, noise=2, ambient_noise_at_signal_0=0.0, ambient_noise_at_signal_1=0.0, ambient_noise_energy_loss=0.0)
    gf, g8, rf, r8 = run(ctx, oracle, cfg, [Seg(echoes([0], [2.0]))], 1, 1)
    f32 = np.float32
    e1, e0 = f32(2.0 * 0.5), f32(2.0 * 0.1)
    want = ((e1 - e0) * f32(1.0) + e0) * f32(cfg.signal_max / 2.0)
    assert (gf[0, 1:] == want).all()
