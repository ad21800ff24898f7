"""The particle filter step of include/radarays_mi355.h (rr_filter_resample, rr_filter_move) restated in numpy: u64 arithmetic and
searchsorted for the resampler, the hash in uint32, the move in np.float32 one operation at a time (numpy's f32 division and square root
are the correctly rounded ones, and nothing is fused).  The GPU tests compare bytes with it; test_filter_host.py holds it to a
brute-force version in Python integers."""
import numpy as np

SUMMARY_DTYPE = np.dtype([("min_sum_d2", "<u8"), ("total_weight", "<u8"), ("sum_w2", "<u8"), ("best", "<u4"), ("n_unique", "<u4")])
VARIATE_VAR = (65536.0 ** 2 - 1.0) / 3.0


def weights(sum_d2, table, quantum):
    """(w uint64 [n], dmin, best)"""
    d2 = np.ascontiguousarray(sum_d2, np.uint64)
    table = np.asarray(table, np.uint16)
    dmin = d2.min()
    idx = np.minimum((d2 - dmin) // np.uint64(quantum), np.uint64(len(table) - 1))
    return table[idx.astype(np.int64)].astype(np.uint64), int(dmin), int(np.argmax(d2 == dmin))


def resample(sum_d2, table, quantum, phase, n_out):
    """-> (cum uint64 [n], ancestors uint32 [n_out], summary SUMMARY_DTYPE scalar)"""
    w, dmin, best = weights(sum_d2, table, quantum)
    n = len(w)
    cum = np.cumsum(w, dtype=np.uint64)
    W = int(cum[-1])
    assert W < 1 << 38 and 0 <= phase < 1 << 24 and 1 <= n_out <= 1 << 22
    r = (phase * W) >> 24
    t = (np.arange(n_out, dtype=np.uint64) * np.uint64(W) + np.uint64(r)) // np.uint64(n_out)
    anc = np.minimum(np.searchsorted(cum, t, side="right"), n - 1).astype(np.uint32)
    s = np.zeros(1, SUMMARY_DTYPE)
    s["min_sum_d2"], s["total_weight"], s["sum_w2"], s["best"] = dmin, W, int((w * w).sum(dtype=np.uint64)), best
    s["n_unique"] = 1 + int(np.count_nonzero(anc[1:] != anc[:-1]))
    return cum, anc, s[0]


def mix32(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def variates(seed, step, n_out):
    """int32 [n_out][3]: v_0, v_1, v_2 of every draw"""
    key = mix32(np.uint32(seed) ^ mix32(np.uint32(step)))
    j = np.arange(n_out, dtype=np.uint32)[:, None] * np.uint32(8) + np.arange(3, dtype=np.uint32)[None, :] * np.uint32(2)
    h, g = mix32(key ^ j), mix32(key ^ (j + np.uint32(1)))
    m = np.uint32(0xffff)
    return ((h & m) + (h >> np.uint32(16)) + (g & m) + (g >> np.uint32(16))).astype(np.int64).astype(np.int32) - np.int32(131070)


def move(states, ancestors, increment, sigma_xy, sigma_t, seed, step):
    """states f32 [n][4], ancestors [n_out] or None, increment (Dc, Ds, dx, dy) -> f32 [n_out][4], the header's expression in its order"""
    st = np.ascontiguousarray(states, np.float32)
    a = np.arange(len(st)) if ancestors is None else np.minimum(np.asarray(ancestors).astype(np.int64), len(st) - 1)
    f = np.float32
    Dc, Ds, dx, dy = (f(x) for x in increment)
    sxy, sgt = f(sigma_xy), f(sigma_t)
    v = variates(seed, step, len(a)).astype(np.float32)
    c, s, tx, ty = (st[a, k] for k in range(4))
    with np.errstate(all="ignore"):
        nx, ny, t = v[:, 0] * sxy, v[:, 1] * sxy, v[:, 2] * sgt
        ux, uy = dx + nx, dy + ny
        txo = (c * ux - s * uy) + tx
        tyo = (s * ux + c * uy) + ty
        q = t * t
        den = f(1.0) + q
        nc, ns = (f(1.0) - q) / den, (t + t) / den
        rc, rs = Dc * nc - Ds * ns, Ds * nc + Dc * ns
        c1, s1 = c * rc - s * rs, s * rc + c * rs
        m = np.sqrt(c1 * c1 + s1 * s1)
        out = np.stack([c1 / m, s1 / m, txo, tyo], axis=1)
    assert out.dtype == np.float32
    return np.ascontiguousarray(out)


# ---- brute force in Python integers, for small cases
def resample_brute(sum_d2, table, quantum, phase, n_out):
    d2 = [int(x) for x in sum_d2]
    dmin = min(d2)
    w = [int(table[min(len(table) - 1, (x - dmin) // quantum)]) for x in d2]
    cum, run = [], 0
    for x in w:
        run += x
        cum.append(run)
    W = cum[-1]
    r = (phase * W) >> 24
    anc = [min(len(d2) - 1, sum(1 for x in cum if x <= (j * W + r) // n_out)) for j in range(n_out)]
    return cum, anc, dict(min_sum_d2=dmin, total_weight=W, sum_w2=sum(x * x for x in w), best=d2.index(dmin), n_unique=len(set(anc)))


def mix32_int(x):
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def variates_brute(seed, step, n_out):
    key = mix32_int(seed ^ mix32_int(step))
    out = []
    for j in range(n_out):
        row = []
        for k in range(3):
            h, g = mix32_int(key ^ ((8 * j + 2 * k) & 0xffffffff)), mix32_int(key ^ ((8 * j + 2 * k + 1) & 0xffffffff))
            row.append((h & 0xffff) + (h >> 16) + (g & 0xffff) + (g >> 16) - 131070)
        out.append(row)
    return out


# ---- one whole step, and the closed loop of the host and GPU tests.  The room, the field, the scan and the poses A and B are those of
# tests/field_ref.py; 4,096 particles start uniformly within +-1 m and +-4 degrees of A (seeded numpy) and run LOOP_STEPS steps of score,
# resample and move with no odometry.  The first values tried were 6 steps, 0.05 m and 0.5 degrees; DESIGN.md §25 says whether they held.
LOOP_PARTICLES, LOOP_STEPS, LOOP_SEED = 4096, 6, 20
LOOP_SIGMA_XY, LOOP_SIGMA_YAW = 0.05, np.radians(0.5)
LOOP_SIGMA_CELLS, LOOP_QUANTUM, LOOP_N_TABLE = 3.0, 1, 1024            # weights exp(-d / 18) over 0..1023 units of sum_d2 above the best


def step(score, states, table, quantum, phase, increment, sigma_xy, sigma_t, seed, step_no):
    """score: states -> FIELD_DTYPE records.  -> (recs, cum, ancestors, summary, the moved states)"""
    recs = score(states)
    cum, anc, summary = resample(recs["sum_d2"], table, quantum, phase, len(recs))
    return recs, cum, anc, summary, move(states, anc, increment, sigma_xy, sigma_t, seed, step_no)


def loop_particles():
    import field_ref as F
    import icp_ref
    rs = np.random.RandomState(LOOP_SEED)
    x = icp_ref.LOOP_A[0] + rs.uniform(-F.LOOP_HALF_XY, F.LOOP_HALF_XY, LOOP_PARTICLES)
    y = icp_ref.LOOP_A[1] + rs.uniform(-F.LOOP_HALF_XY, F.LOOP_HALF_XY, LOOP_PARTICLES)
    yaw = icp_ref.LOOP_A[2] + rs.uniform(-F.LOOP_HALF_YAW, F.LOOP_HALF_YAW, LOOP_PARTICLES)
    return np.stack([np.cos(yaw), np.sin(yaw), x, y], axis=1).astype(np.float32)


def loop_phase(k):
    """where the comb starts in step k: any fixed sequence will do, this one is the hash's"""
    return int(mix32(np.uint32(k))) & 0xffffff


def loop_bound(state, rec, node_xyz, node_sum_d2, slack_steps=0):
    """the closed loop's statement: the particle lies within (1 + slack_steps) lattice steps of §23's argmin node on every axis, and scores
    no worse than it.  -> (|dx|, |dy| in metres, |dyaw| in radians)"""
    import math
    import field_ref as F
    yaw = math.atan2(float(state[1]), float(state[0]))
    d = yaw - float(node_xyz[2])
    ex, ey, eyaw = abs(float(state[2]) - float(node_xyz[0])), abs(float(state[3]) - float(node_xyz[1])), abs(math.atan2(math.sin(d), math.cos(d)))
    k = 1 + slack_steps
    assert ex <= k * F.LOOP_STEP_XY and ey <= k * F.LOOP_STEP_XY and eyaw <= k * F.LOOP_STEP_YAW + 1e-12, (ex, ey, math.degrees(eyaw))
    assert int(rec["sum_d2"]) <= int(node_sum_d2), (int(rec["sum_d2"]), int(node_sum_d2))
    return ex, ey, eyaw
