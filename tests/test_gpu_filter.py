"""The particle filter step on the GPU (rr_filter.hip) against the numpy restatement of its definition (tests/filter_ref.py), as raw bytes:
cum, the ancestors and the summary with n at the edges of the scan tile, n_out below, at and above n, the comb's phase and the quantum at
both ends, sum_d2 up to 2^33 and four shapes of weights; the moved states with and without ancestors, increment and diffusion, and a NaN
state; the host forms; every refusal with the outputs untouched; and RadarHIP.filterStep on the GPU's own images against the three
restatements chained, with the closed loop of tests/test_filter_host.py."""
import ctypes as C
import math

import numpy as np
import pytest

import field_ref as F
import filter_ref as R
import icp_ref
from common import golden_beams
from radarays_ros_amd import native, params, radar
from test_gpu_field import GUARD, dev, guarded, loop_context, payload

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
SHAPES = ("equal", "dominant", "zero_tail", "all_zero")


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    c.set_config(params.kaist_preset(n_cells=64), 16)
    return c


@pytest.fixture(scope="module")
def tiles():
    return native.filter_tile_sizes()


def weights_case(rs, n, shape, quantum):
    """(sum_d2 uint64 [n] reaching 2^33, table uint16 [n_table], n_table)"""
    n_table = 4 if quantum > 1 else 4096
    table = native.filter_weight_table(2.0 if quantum > 1 else 900.0, 1, n_table)
    top = np.uint64(1 << 33)
    span = min(1 << 33, quantum * n_table * 3 // 2)
    d2 = top - rs.randint(0, span + 1, n).astype(np.uint64)
    d2[rs.randint(n)] = top
    if shape == "equal":
        d2[:] = top
    elif shape == "dominant":
        table[1:] = 0
        d2 = top - rs.randint(0, span - quantum + 1, n).astype(np.uint64)
        d2[rs.randint(n)] = top - np.uint64(span)                       # alone in the table's first step ...
        # ... every other one at least a quantum above it, on entries that weigh nothing
    elif shape == "zero_tail":
        table[n_table // 2:] = 0
    elif shape == "all_zero":
        table[:] = 0
    return d2, table, n_table


def run_resample(c, d2, table, n_out, fc, stream=None):
    """the device form on guarded buffers -> (cum bytes, ancestor bytes, summary bytes)"""
    n = len(d2)
    recs = np.zeros(n, native.FIELD_DTYPE)
    recs["sum_d2"], recs["n_in"], recs["n_hit"] = d2, 0xdeadbeef, 0x12345678      # the other fields are not read
    d_recs, d_table = dev(recs), dev(table)
    d_cum, d_anc, d_sum = guarded(8 * n), guarded(4 * n_out), guarded(32)
    torch.cuda.synchronize()
    c.filter_resample_device(d_recs.data_ptr(), n, d_table.data_ptr(), n_out, fc, d_cum.data_ptr(), d_anc.data_ptr(), d_sum.data_ptr(), stream)
    torch.cuda.synchronize()
    return payload(d_cum, 8 * n).tobytes(), payload(d_anc, 4 * n_out).tobytes(), payload(d_sum, 32).tobytes()


def want_resample(d2, table, quantum, phase, n_out):
    cum, anc, s = R.resample(d2, table, quantum, phase, n_out)
    return cum.tobytes(), anc.tobytes(), s.tobytes()


def n_list(tiles):
    t = tiles[0]
    return [1, 2, 63, 64, 65, t - 1, t, t + 1, 2 * t + 1, 65 * t + 3]


@pytest.mark.parametrize("k", range(10))
def test_resampling_is_the_restatement_byte_for_byte(ctx, tiles, k):
    n = n_list(tiles)[k]
    rs = np.random.RandomState(100 + k)
    runs = 0
    for quantum in (1, 1 << 31):
        for shape in SHAPES:
            d2, table, n_table = weights_case(rs, n, shape, quantum)
            for n_out in sorted({1, max(1, n // 2), n, min(2 * n, 1 << 22)}):
                for phase in (0, (1 << 24) - 1):
                    fc = native.filter_config(0.0, 0.0, quantum, n_table, phase, 1, 2)
                    got, want = run_resample(ctx, d2, table, n_out, fc), want_resample(d2, table, quantum, phase, n_out)
                    for name, g, w in zip(("cum", "ancestors", "summary"), got, want):
                        assert g == w, (name, n, n_out, phase, quantum, shape)
                    runs += 1
    assert runs >= 2 * 4 * 1 * 2


def test_resampling_at_the_largest_n(ctx):
    n = 1 << 22
    rs = np.random.RandomState(7)
    d2, table, n_table = weights_case(rs, n, "zero_tail", 1)
    phase = (1 << 24) - 1
    fc = native.filter_config(0.0, 0.0, 1, n_table, phase, 1, 2)
    got, want = run_resample(ctx, d2, table, n, fc), want_resample(d2, table, 1, phase, n)
    assert int(np.frombuffer(want[2], R.SUMMARY_DTYPE)["total_weight"][0]) > 1 << 32         # the sums need their 64 bits
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]


def some_states(rs, n):
    yaw = rs.uniform(-math.pi, math.pi, n)
    return np.stack([np.cos(yaw), np.sin(yaw), rs.uniform(-40, 40, n), rs.uniform(-40, 40, n)], axis=1).astype(np.float32)


def run_move(c, st, anc, inc, fc, stream=None):
    n_out = len(st) if anc is None else len(anc)
    d_in, d_anc, d_out = dev(st), (None if anc is None else dev(anc)), guarded(16 * n_out)
    torch.cuda.synchronize()
    c.filter_move_device(d_in.data_ptr(), len(st), None if anc is None else d_anc.data_ptr(), n_out, inc, fc, d_out.data_ptr(), stream)
    torch.cuda.synchronize()
    return payload(d_out, 16 * n_out).tobytes()


def test_the_move_is_the_restatement_byte_for_byte(ctx):
    rs = np.random.RandomState(21)
    n = 2 * 256 + 37
    st = some_states(rs, n)
    st[11] = (np.nan, 0.5, 1.0, 2.0)                                   # a NaN state passes through
    st[12] = (0.6, 0.8, np.inf, 2.0)
    inc = (math.cos(0.07), math.sin(0.07), 0.31, -0.12)
    for anc in (None, np.sort(rs.randint(0, n, 3 * 256 + 5)).astype(np.uint32), np.arange(n - 1, -1, -1, dtype=np.uint32)[:100]):
        for increment in (None, inc):
            for sxy, syaw in ((0.0, 0.0), (0.05, math.radians(0.5)), (3.0, 1.0)):
                fc = native.filter_config(sxy, syaw, 1, 1, 0, 0x9e3779b9, 41)
                want = R.move(st, anc, (1, 0, 0, 0) if increment is None else increment, fc.sigma_xy, fc.sigma_t, fc.seed, fc.step)
                got = run_move(ctx, st, anc, increment, fc)
                assert got == want.tobytes(), (None if anc is None else len(anc), increment, sxy)
                if anc is None:
                    assert np.all(np.isnan(want[11][:2])) and not np.any(np.isnan(want[13]))
    # sigma 0, no increment: the states copied through the ancestors, (c, s) renormalised
    fc = native.filter_config(0.0, 0.0, 1, 1)
    anc = rs.randint(0, n, 64).astype(np.uint32)
    anc = anc[(anc != 11) & (anc != 12)]
    out = np.frombuffer(run_move(ctx, st, anc, None, fc), np.float32).reshape(-1, 4)
    assert np.array_equal(out[:, 2:], st[anc][:, 2:]) and np.allclose(out[:, :2], st[anc][:, :2], atol=2e-7)
    # another step, another seed: other noise
    a, b, s = (run_move(ctx, st, None, None, native.filter_config(0.05, 0.01, 1, 1, 0, sd, sp)) for sd, sp in ((1, 1), (1, 2), (2, 1)))
    assert a != b and a != s and b != s


def test_host_forms_equal_the_device_forms(ctx, tiles):
    rs = np.random.RandomState(33)
    n = tiles[0] + 77
    d2, table, n_table = weights_case(rs, n, "zero_tail", 1)
    fc = native.filter_config(0.05, 0.01, 1, n_table, 54321, 3, 4)
    recs = np.zeros(n, native.FIELD_DTYPE)
    recs["sum_d2"] = d2
    cum, anc, s = ctx.filter_resample(recs, table, n + 5, fc)
    want = want_resample(d2, table, 1, 54321, n + 5)
    assert (cum.tobytes(), anc.tobytes(), s.tobytes()) == want == run_resample(ctx, d2, table, n + 5, fc)
    st = some_states(rs, n)
    inc = (0.8, 0.6, 1.0, -1.0)
    for a in (None, anc):
        out = ctx.filter_move(st, a, inc, fc)
        assert out.tobytes() == R.move(st, a, inc, fc.sigma_xy, fc.sigma_t, 3, 4).tobytes() == run_move(ctx, st, a, inc, fc)


def test_refusals_write_nothing(ctx):
    L, h = ctx._L, ctx._h
    d = torch.full((1 << 16,), GUARD, dtype=torch.uint8, device=DEV)
    p = d.data_ptr()
    assert p % 256 == 0
    recs, table, cum, anc, summ, sin, sout = p, p + 4096, p + 8192, p + 16384, p + 20480, p + 24576, p + 32768
    ok = native.filter_config(0.1, 0.01, 4, 16, 3, 1, 2)

    def cfg(**kw):
        c = native.RRFilterConfig(ok.quantum, ok.n_table, ok.phase, ok.seed, ok.step, ok.sigma_xy, ok.sigma_t, 0)
        for k, v in kw.items():
            setattr(c, k, v)
        return C.byref(c)

    bad_cfgs = [cfg(quantum=0), cfg(quantum=(1 << 31) + 1), cfg(n_table=0), cfg(n_table=4097), cfg(phase=1 << 24), cfg(reserved=1),
                cfg(sigma_xy=float("nan")), cfg(sigma_xy=-1.0), cfg(sigma_t=float("inf")), cfg(sigma_t=-0.5), None]
    res = lambda *a: L.rr_filter_resample_device(*a)                   # noqa: E731
    mov = lambda *a: L.rr_filter_move_device(*a)                       # noqa: E731
    assert res(None, recs, 8, table, 8, cfg(), cum, anc, summ, None) == -1
    assert mov(None, sin, 8, anc, 8, 1.0, 0.0, 0.0, 0.0, cfg(), sout, None) == -1
    assert L.rr_filter_resample(None, recs, 8, table, 8, cfg(), cum, anc, summ) == -1
    assert L.rr_filter_move(None, sin, 8, anc, 8, 1.0, 0.0, 0.0, 0.0, cfg(), sout) == -1
    calls = []
    for k in range(5):                                                 # each required buffer null
        a = [recs, table, cum, anc, summ]
        a[k] = None
        calls.append(lambda a=a: res(h, a[0], 8, a[1], 8, cfg(), a[2], a[3], a[4], None))
    for n, n_out in ((0, 8), (8, 0), ((1 << 22) + 1, 8), (8, (1 << 22) + 1), (-1, 8)):
        calls.append(lambda n=n, n_out=n_out: res(h, recs, n, table, n_out, cfg(), cum, anc, summ, None))
        calls.append(lambda n=n, n_out=n_out: mov(h, sin, n, anc, n_out, 1.0, 0.0, 0.0, 0.0, cfg(), sout, None))
    for b in bad_cfgs:
        calls.append(lambda b=b: res(h, recs, 8, table, 8, b, cum, anc, summ, None))
        calls.append(lambda b=b: mov(h, sin, 8, anc, 8, 1.0, 0.0, 0.0, 0.0, b, sout, None))
    calls.append(lambda: res(h, recs + 4, 8, table, 8, cfg(), cum, anc, summ, None))                   # misaligned
    calls.append(lambda: res(h, recs, 8, table + 1, 8, cfg(), cum, anc, summ, None))
    calls.append(lambda: res(h, recs, 8, table, 8, cfg(), cum + 4, anc, summ, None))
    calls.append(lambda: res(h, recs, 8, table, 8, cfg(), cum, anc + 2, summ, None))
    calls.append(lambda: res(h, recs, 8, table, 8, cfg(), cum, anc, summ + 4, None))
    calls.append(lambda: mov(h, None, 8, anc, 8, 1.0, 0.0, 0.0, 0.0, cfg(), sout, None))
    calls.append(lambda: mov(h, sin, 8, anc, 8, 1.0, 0.0, 0.0, 0.0, cfg(), None, None))
    calls.append(lambda: mov(h, sin + 8, 8, anc, 8, 1.0, 0.0, 0.0, 0.0, cfg(), sout, None))
    calls.append(lambda: mov(h, sin, 8, anc, 8, 1.0, 0.0, 0.0, 0.0, cfg(), sout + 4, None))
    calls.append(lambda: mov(h, sin, 8, anc + 1, 8, 1.0, 0.0, 0.0, 0.0, cfg(), sout, None))
    calls.append(lambda: mov(h, sin, 8, None, 9, 1.0, 0.0, 0.0, 0.0, cfg(), sout, None))               # more draws than states, no ancestors
    calls.append(lambda: mov(h, sin, 8, anc, 8, 1.0, 0.0, 0.0, 0.0, cfg(), sin, None))                 # aliased
    calls.append(lambda: mov(h, sin, 8, anc, 8, 1.0, 0.0, 0.0, 0.0, cfg(), sin + 64, None))            # overlapping
    calls.append(lambda: mov(h, sin + 64, 8, anc, 8, 1.0, 0.0, 0.0, 0.0, cfg(), sin, None))
    for inc in ((float("nan"), 0.0, 0.0, 0.0), (1.0, float("inf"), 0.0, 0.0), (1.0, 0.0, float("-inf"), 0.0), (1.0, 0.0, 0.0, float("nan"))):
        calls.append(lambda inc=inc: mov(h, sin, 8, anc, 8, *inc, cfg(), sout, None))
    for call in calls:
        assert call() == -3
        assert len(L.rr_last_error(h)) > 0
    # the host forms refuse the same way
    hrecs, htable, hcum, hanc, hsum = np.zeros(8, native.FIELD_DTYPE), np.ones(16, np.uint16), np.full(8, 7, np.uint64), np.full(8, 7, np.uint32), np.full(4, 7, np.uint64)
    assert L.rr_filter_resample(h, hrecs.ctypes.data, 8, htable.ctypes.data, 8, cfg(reserved=1), hcum.ctypes.data, hanc.ctypes.data, hsum.ctypes.data) == -3
    assert L.rr_filter_resample(h, hrecs.ctypes.data, 8, None, 8, cfg(), hcum.ctypes.data, hanc.ctypes.data, hsum.ctypes.data) == -3
    hin, hout = np.zeros((8, 4), np.float32), np.full((8, 4), 7, np.float32)
    assert L.rr_filter_move(h, hin.ctypes.data, 8, None, 8, float("nan"), 0.0, 0.0, 0.0, cfg(), hout.ctypes.data) == -3
    assert L.rr_filter_move(h, hin.ctypes.data, 8, None, 8, 1.0, 0.0, 0.0, 0.0, cfg(), hin.ctypes.data) == -3
    assert np.all(hcum == 7) and np.all(hanc == 7) and np.all(hsum == 7) and np.all(hout == 7)
    torch.cuda.synchronize()
    assert bool((d == GUARD).all())                                    # nothing was written by any of them


def loop_radar():
    s = icp_ref.loop_scene()
    r = radar.RadarHIP(s["verts"], s["faces"], s["face_object_id"])
    r.loadParams(params.kaist_materials(), s["object_materials"], 0)
    r.updateDynCfg(icp_ref.loop_cfg())
    r.setBeamSamples(golden_beams(icp_ref.LOOP_SAMPLES))
    return r


def test_filter_step_is_the_three_restatements_chained_and_closes_the_loop():
    c, _ = loop_context()
    imgs = np.stack([c.simulate(icp_ref.loop_pose(p))[0] for p in (icp_ref.LOOP_A, icp_ref.LOOP_B)])
    pts, offs = c.detect(imgs, icp_ref.LOOP_DET)
    cfg = F.loop_field_cfg()
    fld = c.distance_field(c.rasterize_points([pts[0]], offs[:1], cfg, F.loop_map_state()), cfg)
    scan = pts[1]
    states, xyz = F.loop_lattice()
    rec = c.score_poses(scan, states, fld, cfg)
    node = int(np.argmin(rec["sum_d2"]))
    table = native.filter_weight_table(R.LOOP_SIGMA_CELLS, R.LOOP_QUANTUM, R.LOOP_N_TABLE)
    r = loop_radar()
    d_field, d_table = torch.from_numpy(fld.view(np.int16)).to(DEV), torch.from_numpy(table.view(np.int16)).to(DEV)
    st = torch.from_numpy(R.loop_particles()).to(DEV)
    summary = None
    for k in range(R.LOOP_STEPS + 1):                                  # the last step scores the particles the loop ends with
        fc = native.filter_config(R.LOOP_SIGMA_XY, R.LOOP_SIGMA_YAW, R.LOOP_QUANTUM, R.LOOP_N_TABLE, R.loop_phase(k), R.LOOP_SEED, k)
        before = st.cpu().numpy()
        st, summary = r.filterStep(scan, st, d_field, cfg, d_table, fc)
        recs, cum, anc, want, moved = R.step(lambda x: F.score(scan, x, fld, cfg), before, table, R.LOOP_QUANTUM, R.loop_phase(k), (1, 0, 0, 0),
                                             fc.sigma_xy, fc.sigma_t, R.LOOP_SEED, k)
        assert r.m_filter["recs"].cpu().numpy().tobytes() == recs.tobytes(), k
        assert r.m_filter["cum"].cpu().numpy().tobytes() == cum.tobytes(), k
        assert r.m_filter["ancestors"].cpu().numpy().tobytes() == anc.tobytes(), k
        assert summary.tobytes() == want.tobytes(), k
        assert st.cpu().numpy().tobytes() == moved.tobytes(), k
    best = int(summary["best"])
    assert int(summary["min_sum_d2"]) == int(recs["sum_d2"][best])
    ex, ey, eyaw = R.loop_bound(before[best], recs[best], xyz[node], rec["sum_d2"][node], slack_steps=1)
    print("closed loop on the GPU: §23's node (%.2f m, %.2f m, %.1f deg) at sum_d2 %d; after %d steps the best particle scores %d, %.3f m, %.3f m, "
          "%.2f deg from the node" % (xyz[node][0], xyz[node][1], math.degrees(xyz[node][2]), rec["sum_d2"][node], R.LOOP_STEPS,
                                      int(summary["min_sum_d2"]), ex, ey, math.degrees(eyaw)))
    # the caller's rule: a previous summary whose effective sample size is above the floor keeps every particle
    fc = native.filter_config(R.LOOP_SIGMA_XY, R.LOOP_SIGMA_YAW, R.LOOP_QUANTUM, R.LOOP_N_TABLE, 0, R.LOOP_SEED, 99)
    assert radar.RadarHIP.effectiveSampleSize(summary) > 100
    kept, s2 = r.filterStep(scan, st, fld, cfg, table, fc, increment=(1.0, 0.0, 0.1, 0.0), n_eff_floor=100, prev_summary=summary)
    assert kept.cpu().numpy().tobytes() == R.move(st.cpu().numpy(), None, (1.0, 0.0, 0.1, 0.0), fc.sigma_xy, fc.sigma_t, R.LOOP_SEED, 99).tobytes()
    drawn, s3 = r.filterStep(scan, st, fld, cfg, table, fc, increment=(1.0, 0.0, 0.1, 0.0), n_eff_floor=1e9, prev_summary=summary)
    assert s2.tobytes() == s3.tobytes() and drawn.cpu().numpy().tobytes() != kept.cpu().numpy().tobytes()
