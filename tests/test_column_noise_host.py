"""The precondition of tests/test_gpu_column_noise.py, on the CPU.  The one licensed difference between k_column's noise path and
the oracle's is the fourth power of the amplitude law: the oracle calls pow(signal_, 4.0) (RadarCPU.cpp:509), the kernel squares
twice.  signal_ is an f32, so its square is exact in f64 and the second product is the correctly rounded fourth power; libm's pow
is within an ulp of it, and the two can narrow to different f32 only where the exact power lies within that of an f32 rounding
boundary.  For the inputs of the GPU tests that is checked here, bin by bin: it is a condition on the inputs, not a tolerance.

The slice the law is evaluated on is column_noise_cases.replay, a numpy restatement of RadarCPU.cpp:402-450; it is tied to
orc_column first (noise off: the f32 column is slice * energy_max * signal_max / max_val)."""
import numpy as np
import pytest

import column_noise_cases as cases
from test_gpu_column import config

E_FLAT = 0.3
N_CELLS = [1, 63, 64, 65, 200, 513, 8192]


def slices_of(oracle, cfg, segs):
    """replay of every segment, held to orc_column bit for bit"""
    smear, mode = cases.smear_of(oracle, cfg)
    off = cfg.copy(ambient_noise=0)
    out = []
    for s in segs:
        sl, max_val = cases.replay(cfg, smear, mode, s.list)
        rf, _ = oracle.column(off, s.list["cell"], s.list["strength"])
        with np.errstate(all="ignore"):
            mine = sl * np.float32(cfg.energy_max) * np.float32(cfg.signal_max / np.float64(max_val))
        assert np.array_equal(mine, rf, equal_nan=True), np.flatnonzero(mine.view(np.uint32) != rf.view(np.uint32))[:8]
        out.append((sl, max_val))
    return out


def assert_powers_agree(cfg, sl, max_val, what):
    x, by_power, by_libm, by_squaring = cases.fourth_powers(cfg, sl, max_val)
    bad = (by_power.view(np.uint32) != by_squaring.view(np.uint32)) | (by_libm.view(np.uint32) != by_squaring.view(np.uint32))
    assert not bad.any(), (what, x[bad][:4].tolist())
    return x


@pytest.mark.parametrize("n_cells", N_CELLS)
def test_dyadic_columns_have_exact_fourth_powers(oracle, n_cells):
    """Step 1's columns.  Without a denoiser signal_ is (32 - k) / 32: at most five significant bits, a fourth power of at most 20
    -- exact in f64 however it is formed.  The two tri9 columns hold what a window leaves: checked like step 3's."""
    kinds = cases.column_kinds(n_cells, seed=n_cells)
    assert len(kinds) == 8
    for name, s in kinds.items():
        cfg = config(n_cells, noise=2, **cases.den_of(name))
        (sl, max_val), = slices_of(oracle, cfg, [s])
        x = assert_powers_agree(cfg, sl, max_val, name)
        if not cases.den_of(name) and len(x):
            assert max_val == np.float32(cases.PEAK) and np.array_equal(x * 32, np.round(x * 32)) and x.min() >= 0.5, name
    # what the kinds are for
    nz = {name: np.flatnonzero(slices_of(oracle, config(n_cells, **cases.den_of(name)), [s])[0][0]) for name, s in kinds.items()}
    assert nz["bin_0"].tolist() == [0] and nz["last_bin"].tolist() == [n_cells - 1] and len(nz["one_echo"]) == 1
    assert len(nz["falls_to_zero"]) == 0 and len(kinds["falls_to_zero"].list) == 2
    if n_cells >= 63:
        assert len(nz["falls_to_zero_beside_echoes"]) > 0 and len(np.unique(nz["one_tile"] // 64)) == 1
        assert len(nz["last_bin_of_tiles"]) and all(b % 64 == 63 or b == n_cells - 1 for b in nz["last_bin_of_tiles"])
        assert len(np.unique(nz["every_tile"] // 64)) == (n_cells + 63) // 64
        sl, max_val = slices_of(oracle, config(n_cells, **cases.TRI9), [kinds["falls_to_zero"]])[0]
        assert max_val > 0 and not sl.any()                          # risen, and back at exactly 0.0f


@pytest.mark.parametrize("key", sorted(cases.RANDOM_SEEDS), ids=lambda k: "%s-%d" % k)
def test_random_columns_meet_the_precondition(oracle, key):
    """Step 3's columns under their seeds: in every non-empty bin numpy's power, libm's pow and the two squarings give the same f32."""
    den, n_cells = key
    cfg = config(n_cells, noise=2, **cases.DENOISERS[den])
    segs = cases.random_columns(cases.RANDOM_SEEDS[key], n_cells)
    n = 0
    for k, (sl, max_val) in enumerate(slices_of(oracle, cfg, segs)):
        n += len(assert_powers_agree(cfg, sl, max_val, (key, k)))
    assert n > 100


def test_amplitude_law_in_numpy_is_the_oracles(oracle):
    """fourth_powers feeds the law of RadarCPU.cpp:497-512; restated whole, it gives orc_noise_amplitude's f32"""
    cfg = config(200, noise=2, **cases.TRI9)
    s = cases.random_columns(5, 200)[2]
    (sl, max_val), = slices_of(oracle, cfg, [s])
    x, by_power, by_libm, by_squaring = cases.fourth_powers(cfg, sl, max_val)
    n0 = np.float32(np.float64(max_val) * cfg.ambient_noise_at_signal_0)
    n1 = np.float32(np.float64(max_val) * cfg.ambient_noise_at_signal_1)
    amp = ((by_squaring * n0).astype(np.float64) + (1.0 - by_squaring.astype(np.float64)) * np.float64(n1)).astype(np.float32)
    signal = sl[sl != 0] * np.float32(cfg.energy_max)
    want = np.float32([oracle.noise_amplitude(float(v), float(max_val), cfg.ambient_noise_at_signal_0, cfg.ambient_noise_at_signal_1)
                       for v in signal])
    assert np.array_equal(amp.view(np.uint32), want.view(np.uint32))


def test_offsets_and_layouts_are_what_the_issue_names():
    cols = sorted({c for lay in cases.LAYOUTS for c in cases.layout_columns(lay)})
    assert {0, 5, 20, 100, 399} <= set(cols)
    assert any(az > 0 and sc > 0 for az, sc, _ in cases.LAYOUTS)
    for noise in (1, 2):
        off = cases.offsets_of(noise)
        assert np.isfinite(off).all() and (np.abs(off.astype(np.float64)) < 2.0 ** 31).all()
    off = cases.offsets_of(2).astype(np.float64)
    assert any(np.floor(o) % 256 == 255 and np.floor(o + 0.05) % 256 == 0 for o in off)          # X wraps between bins 0 and 1
    assert (off < 0).any() and (off == np.floor(off)).sum() >= 3
    assert np.float32(-3.7) in cases.offsets_of(1) and np.float32(2147483520.0) in cases.offsets_of(1)
    assert 5 * 0.2 == 1.0 and 20 * 0.05 == 1.0                       # the y = 0 lattice row, in f64 as both sides form it
