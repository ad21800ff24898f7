"""The bounce loop of ONE azimuth, restated in Python: the wave list of rr_simulate_paths (include/radarays_mi355.h, "wave paths") and
the azimuth's echo stream.  Built only on what the oracle exports per hit -- Scene.intersect, oracle.fresnel,
oracle.back_reflection_shader, orc_incidence_angle (the reference's acosf) -- with numpy f32 / f64 for the rest: the azimuth's frame,
move, the normal convention, material select, pruning at the threshold, skip_dist and the cell (RadarCPU.cpp:184-380, 410-413, in the
operation order of oracle/radarays_oracle.c).  tests/test_paths_host.py pins it to the oracle's extended echo log; tests/test_gpu_paths.py
holds the GPU's records to it."""
import ctypes as C

import numpy as np

from radarays_ros_amd.native import WAVE_DTYPE

F = np.float32
NONE = 0xFFFFFFFF
SKIP_DIST = F(0.001)          # RadarCPU.cpp:374
ECHO_REF_DTYPE = np.dtype([("cell", "<i4"), ("strength", "<f4"), ("face", "<u4"), ("pass", "u1"), ("kind", "u1"), ("wave", "<i4")])


def q_mul(a, b):
    """rmagine Quaternion * Quaternion, (x, y, z, w) of f32, term order as in rmagine"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return (aw * bx + ax * bw + ay * bz - az * by,
            aw * by - ax * bz + ay * bw + az * bx,
            aw * bz + ax * by - ay * bx + az * bw,
            aw * bw - ax * bx - ay * by - az * bz)


def q_inv(a):
    return (-a[0], -a[1], -a[2], a[3])


def q_rot(q, v):
    """rmagine Quaternion * Vector = (q (v, 0) q^-1).xyz"""
    return q_mul(q_mul(q, (v[0], v[1], v[2], F(0.0))), q_inv(q))[:3]


def q_from_yaw(theta):
    """rmagine Quaternion::set(EulerAngles(0, 0, yaw)): cosf / sinf as the correctly rounded f32 of the f64 function"""
    cy, sy = F(np.cos(np.float64(F(theta) / F(2.0)))), F(np.sin(np.float64(F(theta) / F(2.0))))
    cr = cp = F(1.0)
    sr = sp = F(0.0)
    return (sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy)


def v_add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def v_scale(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def v_dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def v_cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def v_norm(a):
    return np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])


def v_normalize(a):
    d = v_norm(a)
    return (a[0] / d, a[1] / d, a[2] / d)


def f3(v):
    return tuple(F(x) for x in v)


def azimuth_frame(pose, az, oc):
    """Tam = Tsm * Tas (RadarCPU.cpp:201-206) -> (q_am, t_am)"""
    p = f3(pose[:4]) + f3(pose[4:7])
    q_sm, t_sm = p[:4], p[4:]
    theta = F(oc.theta_min) + F(az) * F(oc.theta_inc)
    q_am = q_mul(q_sm, q_from_yaw(theta))
    t_am = v_add(q_rot(q_sm, (F(0.0), F(0.0), F(0.0))), t_sm)
    return q_am, t_am


def move(orig, direction, time, distance):
    """Wave::move (radar_types.h:108-113): Vector * double narrows the factor to float; the wave's velocity is always 0.3"""
    return v_add(orig, v_scale(direction, F(distance))), time + float(distance) / 0.3


def cell_of(time, resolution):
    """RadarCPU.cpp:410-413"""
    half_time = F(time / 2.0)
    signal_dist = F(0.3 * float(half_time))
    return int(float(signal_dist) / resolution)


def trace_azimuth(oracle, sc, scene, materials, object_materials, cfg, beam_dirs, pose, az, n_angles=400, map_frame=False):
    """-> (waves WAVE_DTYPE [n], pass_counts [n_reflections], echoes ECHO_REF_DTYPE [m]) of azimuth az.
    sc: the oracle.Scene of `scene` (verts / faces / face_object_id); materials: (velocity, ambient, diffuse, specular) tuples."""
    oc = oracle.make_config(cfg, n_angles)
    L = oracle.lib()
    thr, air, res = float(oc.wave_energy_threshold), int(oc.material_id_air), float(oc.resolution)
    verts, faces = np.asarray(scene["verts"], F), np.asarray(scene["faces"])
    obj_of = np.asarray(scene["face_object_id"])
    q_am, t_am = azimuth_frame(np.asarray(pose, F), az, oc)
    q_ma = q_inv(q_am)
    fp = C.POINTER(C.c_float)

    def arr(v):
        return (C.c_float * 3)(*[float(x) for x in v])

    def incidence_angle(normal, direction):
        return F(L.orc_incidence_angle(C.cast(arr(normal), fp), C.cast(arr(direction), fp)))

    # a wave: (orig, dir, energy, time, material, parent index, branch)
    cur = [((F(0.0), F(0.0), F(0.0)), f3(b), 1.0, 0.0, 0, -1, 0) for b in np.asarray(beam_dirs, F).reshape(-1, 3)]
    recs, echoes, pass_counts = [], [], []
    first = 0
    for pass_id in range(int(oc.n_reflections)):
        pass_counts.append(len(cur))
        nxt = []
        for i, (orig, direction, energy, time, mat, parent, branch) in enumerate(cur):
            o_m, d_m = v_add(q_rot(q_am, orig), t_am), q_rot(q_am, direction)
            hit = sc.intersect(np.array(o_m, F), np.array(d_m, F))
            r = {"echo": -1}
            r["o"], r["d"] = (o_m, d_m) if map_frame else (orig, direction)
            r["energy"], r["time"], r["material"], r["parent"] = energy, time, mat, parent
            info = (pass_id << 24) | (branch << 28)
            if hit is None:     # :252-255 the wave dies silently
                r["range"], r["face"], r["info"] = -1.0, NONE, info | 0xFFFFFF
                recs.append(tuple(r[k] for k in WAVE_DTYPE.names))
                continue
            rng, f, _ = hit
            f = int(f)
            obj_id = int(obj_of[f])
            r["range"], r["face"] = rng, f
            v0, v1, v2 = (f3(verts[k]) for k in faces[f])
            e1, e2 = (v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]), (v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2])
            nint = q_rot(q_ma, v_normalize(v_cross(e1, e2)))
            if v_dot(direction, nint) > F(0.0):
                nint = (-nint[0], -nint[1], -nint[2])
            normal = v_normalize(nint)      # :248
            i_orig, i_time = move(orig, direction, time, np.float64(F(rng)))      # :258
            mat_refr = int(object_materials[obj_id]) if mat == air else air       # :266-280
            v_refr = F(materials[mat_refr][0]) if mat != mat_refr else F(0.3)
            rdir, renergy, tdir, tenergy = oracle.fresnel(np.array(normal, F), np.array(direction, F), energy, 0.5, 0.3, float(v_refr))
            rdir, tdir = f3(rdir), f3(tdir)
            me = len(recs)
            if renergy > thr:       # :288
                nxt.append((i_orig, rdir, renergy, i_time, mat, first + i, 1))
                if mat == air:      # :302
                    _, amb, dif, spe = materials[mat_refr]
                    ang = incidence_angle(normal, direction)
                    if pass_id == 0 or oc.record_multi_reflection:      # :319
                        time_back = F(i_time * 2.0)
                        echoes.append((cell_of(float(time_back), res), oracle.back_reflection_shader(float(ang), float(F(renergy)), amb, dif, spe), f, pass_id, 0, me))
                        info |= 1 << 30
                    if pass_id > 0 and oc.record_multi_path:            # :325-360
                        dist = v_norm(i_orig)
                        dsh = (i_orig[0] / dist, i_orig[1] / dist, i_orig[2] / dist)
                        time_to_sensor = float(dist) / 0.3
                        if float(v_dot(direction, dsh)) > float(oc.multipath_threshold):
                            a2 = incidence_angle(dsh, rdir)             # acosf(dot(-rdir, dsh))
                            echoes.append((cell_of(i_time + time_to_sensor, res), oracle.back_reflection_shader(float(a2), float(F(renergy)), amb, dif, spe), f, pass_id, 1, me))
                            info |= 1 << 31
            if tenergy > thr:       # :367
                nxt.append((i_orig, tdir, tenergy, i_time, mat_refr, first + i, 2))
            r["info"] = info | (obj_id & 0xFFFFFF)
            recs.append(tuple(r[k] for k in WAVE_DTYPE.names))
        first += len(cur)
        cur = [(move(o, d, t, np.float64(SKIP_DIST))[0], d, e, move(o, d, t, np.float64(SKIP_DIST))[1], m, p, b) for o, d, e, t, m, p, b in nxt]      # :374-378
    waves = np.array(recs, WAVE_DTYPE) if recs else np.zeros(0, WAVE_DTYPE)
    ech = np.array(echoes, ECHO_REF_DTYPE) if echoes else np.zeros(0, ECHO_REF_DTYPE)
    k = 0
    while k < len(ech):             # a wave's first echo: its index in the stream
        if waves["echo"][ech["wave"][k]] < 0:
            waves["echo"][ech["wave"][k]] = k
        k += 1
    return waves, np.array(pass_counts, np.int64), ech
