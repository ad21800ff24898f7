"""Place recognition on the card: descriptors of 20 rings x 60 sectors (K = 1200 bytes), databases of 1e5 and
1e6 of them, 1 and 16 queries.

    python tools/probe_place.py [--reps 10] [--rounds 3] [--json out.json]
    python tools/probe_place.py --kernels-only        # the library's calls alone, for rocprofv3 --kernel-trace --stats
    python tools/probe_place.py --build               # also: buildPlaceDatabase in poses per second on config 2

1. rr_match_descriptors_device: a host clock around a synchronous call (launches, the copy of the records and the synchronise
   included), and k_place_match alone from the context's kernel timer where it has one -- here: the call without the full
   outputs, top_k = 8.
2. The byte floor: n_db * K bytes once from HBM at 6.3 TB/s, the rate a float4 copy achieves on this card.
3. What a user would write today with torch: the rolled queries [n_query * S][K] times the database [K][n_db] by fp32 matmul,
   then max over the shifts.  fp32 is NOT exact here (255^2 x 1200 > 2^24); how far its xcorr is from the exact one, and how
   many best-candidate decisions it changes, is reported.
The routes are alternated inside each round; the median over the rounds is reported.  The library's records are compared with
an exact int64 torch computation on a slice of the database before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from radarays_ros_amd import native  # noqa: E402

R, S = 20, 60
K = R * S
N_DB = (100_000, 1_000_000)
N_QUERY = (1, 16)
TOP_K = 8
HBM_BYTES_PER_S = 6.3e12


def timed(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e6


def rolled(q):
    """uint8 [nq][R][S] on the device -> [nq * S][K]: row (q, s) is roll(q, s) along the sectors"""
    return torch.stack([torch.roll(q, s, dims=2) for s in range(S)], dim=1).reshape(-1, K)


def torch_route(rolls_f32, db_f32_t, nq):
    """fp32 xcorr [nq][S][n_db] -> (largest xcorr per pair, its shift)"""
    xc = (rolls_f32 @ db_f32_t).reshape(nq, S, -1)
    return xc.max(dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()

    ctx = native.Context(0)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(13)
    db = torch.randint(0, 256, (max(N_DB), R, S), dtype=torch.uint8, generator=g).to(dev)
    q = torch.randint(0, 256, (max(N_QUERY), R, S), dtype=torch.uint8, generator=g).to(dev)
    q[0] = torch.roll(db[77_777], 9, dims=1)             # found at shift S - 9 with no error
    out = {"n_rings": R, "n_sectors": S, "top_k": TOP_K, "reps": a.reps, "rounds": a.rounds}

    def lib(nq, n):
        return ctx.match_descriptors_device(q.data_ptr(), nq, db.data_ptr(), n, R, S, TOP_K)
    rec = lib(max(N_QUERY), min(N_DB))
    assert rec[0][0]["index"] == 77_777 and rec[0][0]["sse"] == 0 and rec[0][0]["shift"] == S - 9, rec[0][0]
    # exact check on a slice: an f64 matmul on the device (torch has no integer one here), exact because a sum stays below 255^2 K < 2^53
    sl = 4096
    xc = (rolled(q).double() @ db[:sl].reshape(sl, K).double().T).long().reshape(max(N_QUERY), S, sl)
    top = xc.max(dim=1).values
    sse = (q.long() ** 2).sum(dim=(1, 2))[:, None] + (db[:sl].long() ** 2).sum(dim=(1, 2))[None, :] - 2 * top
    d_sse = torch.zeros((max(N_QUERY), sl), dtype=torch.int32, device=dev)
    ctx.match_descriptors_device(q.data_ptr(), max(N_QUERY), db.data_ptr(), sl, R, S, TOP_K, d_sse.data_ptr())
    assert bool((d_sse.long() == sse).all()), "the library's sse differs from the exact int64 product"

    if a.kernels_only:
        for n in N_DB:
            for nq in N_QUERY:
                for _ in range(a.reps):
                    lib(nq, n)
        return emit(out, a)

    for n in N_DB:
        db_t = db[:n].reshape(n, K).float().T.contiguous()
        for nq in N_QUERY:
            rolls = rolled(q[:nq]).float()
            routes = {"match": (lambda: lib(nq, n)), "torch_matmul_fp32": (lambda: torch_route(rolls, db_t, nq))}
            for fn in routes.values():
                fn()
            times = {k: [] for k in routes}
            for _ in range(a.rounds):
                for k, fn in routes.items():
                    times[k].append(timed(fn, a.reps))
            med = {k: round(float(np.median(v)), 1) for k, v in times.items()}
            # how far fp32 is off, on the first 65536 candidates
            m = min(n, 65536)
            exact = (rolled(q[:nq]).double() @ db[:m].reshape(m, K).double().T).long().reshape(nq, S, m)
            approx = (rolls @ db_t[:, :m]).reshape(nq, S, m)
            err = float((approx.double() - exact.double()).abs().max())
            moved = int((approx.argmax(dim=1) != exact.argmax(dim=1)).sum())
            floor_us = n * K / HBM_BYTES_PER_S * 1e6
            out["n_db%d_q%d" % (n, nq)] = {"us": {k: [round(t, 1) for t in v] for k, v in times.items()}, "median_us": med,
                                          "byte_floor_us": round(floor_us, 1), "match_over_floor": round(med["match"] / floor_us, 2),
                                          "torch_over_match": round(med["torch_matmul_fp32"] / med["match"], 2),
                                          "fp32_max_abs_error": err, "fp32_best_shifts_moved": moved, "pairs_checked": nq * m}
            print("n_db = %7d, n_query = %2d: match %.1f us (byte floor %.1f us, x%.1f), torch fp32 matmul %.1f us; fp32 max |error| %.0f, "
                  "%d of %d best shifts moved" % (n, nq, med["match"], floor_us, med["match"] / floor_us, med["torch_matmul_fp32"], err, moved, nq * m),
                  flush=True)
        del db_t
    if a.build:
        out["build"] = build_rate(a)
    return emit(out, a)


def build_rate(a):
    """RadarHIP.buildPlaceDatabase's two routes in poses per second on config 2 (1 pass, 200 rays per beam, noise on), 256 poses, 64
    per call, beside rr_simulate_batch_device alone"""
    from radarays_ros_amd import params, scenes
    from radarays_ros_amd.fixtures import golden_beams, materials_for
    scene = scenes.config_scene(2)
    cfg = params.kaist_preset(n_reflections=1, n_samples=200, ambient_noise=2)
    mats = materials_for(scene)
    ctx = native.Context(0)
    ctx.set_mesh(scene["verts"], scene["faces"], scene["face_object_id"])
    ctx.set_materials(mats, scene["object_materials"], 0)
    ctx.set_config(cfg, params.N_ANGLES)
    ctx.set_beam_samples(golden_beams(200))
    ctx.set_noise_offsets((np.random.RandomState(7).uniform(0, 1, 64 * params.N_ANGLES) * 1000.0).astype(np.float32))
    poses = scenes.trajectory(256, scene["name"])
    imgs = torch.empty((64, cfg.n_cells, params.N_ANGLES), dtype=torch.uint8, device="cuda:0")
    d_desc = torch.empty((256, R, S), dtype=torch.uint8, device="cuda:0")
    place = (R, S)

    def host_route():
        return [ctx.simulate_batch_describe(poses[at:at + 64], place) for at in range(0, 256, 64)]

    def device_route():
        for at in range(0, 256, 64):
            ctx.simulate_batch_device(poses[at:at + 64], imgs.data_ptr())
            ctx.describe_images_device(imgs.data_ptr(), 64, place, d_desc[at:].data_ptr())
        ctx.synchronize()

    def simulate_only():
        for at in range(0, 256, 64):
            ctx.simulate_batch_device(poses[at:at + 64], imgs.data_ptr())
        ctx.synchronize()
    res = {"poses": 256}
    for name, fn in (("simulate_batch_describe", host_route), ("simulate_then_describe_device", device_route), ("simulate_batch_device_alone", simulate_only)):
        fn()
        t = [timed(fn, 1) for _ in range(a.rounds)]
        res[name + "_poses_per_s"] = round(256 / (float(np.median(t)) * 1e-6), 1)
    print("config 2, 256 poses: %s" % res, flush=True)
    return res


def emit(out, a):
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
