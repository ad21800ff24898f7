"""numpy restatement of the Doppler definition (include/radarays_mi355.h, "Doppler"): the range rate v_r of every echo of ONE azimuth,
its shifted cell and the winner column of the velocity image, as a pure function of the azimuth's wave list in the map frame (geometry),
the same list in the sensor frame (times, and the multipath distance |i_orig| as tests/paths_ref.py forms it), the echo stream (order
and strengths), the twists, the sensor's velocity, the gain and the resolution.  f32 throughout, in the operation order the header
states (the v_dot / v_cross term order of tests/paths_ref.py); it never calls the code under test."""
import numpy as np

import labels_ref
import paths_ref as R

F = np.float32
NONE = 0xFFFFFFFF


def _t(a):
    """[n][3] f32 -> the tuple of component arrays paths_ref's vector helpers take"""
    a = np.asarray(a, F)
    return (a[..., 0], a[..., 1], a[..., 2])


def wave_rates(waves_map, twists, v_s):
    """per wave of the list: (dl f32 [n] = dL/dt of a path that ends on the wave's hit, v f32 [n][3] the velocity of its hit point,
    p f32 [n][3] the hit point, u the direction); a wave that missed has v = 0 and carries no echo"""
    w = np.asarray(waves_map)
    n = len(w)
    tw = np.asarray(twists, F).reshape(-1, 6)
    vs = tuple(F(x) for x in np.asarray(v_s, F).reshape(3))
    u = _t(w["d"])
    rng = w["range"].astype(F)
    o = _t(w["o"])
    p = R.v_add(o, R.v_scale(u, rng))                               # p_i = o_i + range_i * u_i
    obj = (w["info"] & np.uint32(0xFFFFFF)).astype(np.int64)
    hit = (rng >= 0) & (obj < len(tw))
    ob = np.where(hit, obj, 0)
    V, Om = _t(tw[ob, :3]), _t(tw[ob, 3:])
    with np.errstate(all="ignore"):
        v = R.v_add(V, R.v_cross(Om, p))                            # v_b(p) = V_b + Omega_b x p
    v = tuple(np.where(hit, c, F(0.0)).astype(F) for c in v)
    pas = ((w["info"] >> np.uint32(24)) & np.uint32(15)).astype(np.int64)
    acc = np.zeros(n, F)
    for k in range(int(pas.max()) + 1 if n else 0):                 # from the beam to the echo: a parent lies one pass earlier
        m = np.flatnonzero(pas == k)
        um = tuple(c[m] for c in u)
        if k == 0:
            acc[m] = -R.v_dot(tuple(np.full(len(m), c, F) for c in vs), um)
        else:
            par = w["parent"][m]
            vp, up = tuple(c[par] for c in v), tuple(c[par] for c in u)
            diff = (up[0] - um[0], up[1] - um[1], up[2] - um[2])    # u_i - u_{i+1}, formed before its dot product
            acc[m] = acc[par] + R.v_dot(vp, diff)
    dl = acc + R.v_dot(v, u)
    assert dl.dtype == F and acc.dtype == F
    return dl, np.stack(v, 1), np.stack(p, 1), np.stack(u, 1)


def signal_dists(waves_sensor):
    """per wave: (signal_dist of its path echo, of its multipath echo), f32 [n] each -- paths_ref.move and paths_ref.cell_of without the
    division by the resolution"""
    w = np.asarray(waves_sensor)
    rng = w["range"].astype(F)
    t_hit = w["time"] + rng.astype(np.float64) / 0.3                # move: time + float(distance) / 0.3

    def dist_of(time):
        half_time = (time / 2.0).astype(F)
        return (0.3 * half_time.astype(np.float64)).astype(F)

    time_back = (t_hit * 2.0).astype(F)
    o, d = _t(w["o"]), _t(w["d"])
    with np.errstate(all="ignore"):
        i_orig = R.v_add(o, R.v_scale(d, rng))
        dist = R.v_norm(i_orig)
        return dist_of(time_back.astype(np.float64)), dist_of(t_hit + dist.astype(np.float64) / 0.3)


def shifted_cells(signal_dist, v_r, gain, resolution):
    """r' = signal_dist + gain * v_r (f32, not fused); cell' = (int)((double)r' / resolution), -1 when the quotient is not in [0, 2^31)"""
    with np.errstate(all="ignore"):
        r = np.asarray(signal_dist, F) + F(gain) * np.asarray(v_r, F)
        assert r.dtype == F
        q = r.astype(np.float64) / float(resolution)
        ok = np.isfinite(q) & (q >= 0.0) & (q < 2147483648.0)
        return np.where(ok, np.trunc(np.where(ok, q, 0.0)), -1).astype(np.int64)


def doppler(waves_map, waves_sensor, n_echoes, twists, v_s, gain, resolution):
    """-> (v_r f32 [n_echoes], cell' int64 [n_echoes], signal_dist f32 [n_echoes]) of one azimuth, indexed like its echo stream"""
    wm, ws = np.asarray(waves_map), np.asarray(waves_sensor)
    dl, v, p, _ = wave_rates(wm, twists, v_s)
    sd0, sd1 = signal_dists(ws)
    e0, e1 = ((wm["info"] >> np.uint32(30)) & np.uint32(1)) > 0, (wm["info"] >> np.uint32(31)) > 0
    vr, sd = np.full(n_echoes, np.nan, F), np.full(n_echoes, np.nan, F)
    i0 = wm["echo"][e0]
    vr[i0], sd[i0] = dl[e0], sd0[e0]                                # path echo: v_r = dL/dt
    if e1.any():                                                    # multipath echo: straight back to the sensor
        t_am = tuple(F(x) for x in wm["o"][0])                      # (pass 0 starts in t_am)
        vs = tuple(F(x) for x in np.asarray(v_s, F).reshape(3))
        pk, vk = _t(p[e1]), _t(v[e1])
        with np.errstate(all="ignore"):
            e = R.v_normalize((pk[0] - t_am[0], pk[1] - t_am[1], pk[2] - t_am[2]))
            back = R.v_dot((vk[0] - vs[0], vk[1] - vs[1], vk[2] - vs[2]), e)
        i1 = (wm["echo"] + e0.astype(np.int32))[e1]
        vr[i1], sd[i1] = F(0.5) * (dl[e1] + back), sd1[e1]
    assert vr.dtype == F and not np.isnan(sd).any()
    return vr, shifted_cells(sd, vr, gain, resolution), sd


def winner_column(cells, strengths, v_r, n_cells, w, mode):
    """the v_r of the echo that wins each bin by the label definition (tests/labels_ref.py) on the shifted cells; NaN: nobody reaches it"""
    n = len(cells)
    idx, _ = labels_ref.label_column_fast(np.clip(cells, -1, 2 ** 31 - 1), strengths, np.arange(n, dtype=np.uint32), np.zeros(n, np.uint32), n_cells, w, mode)
    out = np.full(n_cells, np.nan, F)
    hit = idx != NONE
    out[hit] = np.asarray(v_r, F)[idx[hit]]
    return out
