"""Dynamic scenes on the card: what a pose / vertex update costs, what moving vehicles cost the frame path, how the tree
cost grows along a drive, and what a rebuild costs (BASELINE.md "Dynamic scenes").

    python tools/probe_dynamic.py [--configs 2 3 4] [--vehicles 64] [--steps 20] [--json out.json]
    python tools/probe_dynamic.py --refit-only --configs 4      # the refit calls alone (for rocprofv3 --kernel-trace --stats)

Meshes: the config meshes of bench.py's workloads + `--vehicles` vehicle boxes (scenes.add_vehicles), host-built tree.
Frame path: bench.py's loop shape -- a step = the 16-pose trajectory as two batches of 8 frames delivered to page-locked
host memory (rr_simulate_batch_host_async) -- timed static, then with every vehicle moved before each step."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from radarays_ros_amd import native, params, scenes  # noqa: E402
from radarays_ros_amd.fixtures import golden_beams, materials_for  # noqa: E402

WORKLOAD = {2: (1, 200), 3: (4, 200), 4: (4, 200)}      # config -> (passes, rays per beam), as bench.py's workloads


def yaw_q(yaw):
    return np.array([0.0, 0.0, np.sin(yaw / 2.0), np.cos(yaw / 2.0)], np.float32)


def rot_z(yaw, p):
    c, s = np.cos(yaw), np.sin(yaw)
    return np.array([c * p[0] - s * p[1], s * p[0] + c * p[1], p[2]], np.float64)


def drive_poses(scene, n_obj, dist, heading):
    """every vehicle driven `dist` metres along its own heading (a straight drive through the map; terrain not followed)"""
    P = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float32), (n_obj, 1))
    for oid, cen, h in zip(scene["vehicle_objects"], scene["vehicle_centers"], heading):
        P[oid, 4:] = np.array([np.cos(h), np.sin(h), 0.0], np.float32) * np.float32(dist)
    return P


def jitter_poses(scene, n_obj, k, rs):
    """step k: every vehicle turned and shifted a little around its rest place (traffic that stays in view)"""
    P = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float32), (n_obj, 1))
    for oid, cen in zip(scene["vehicle_objects"], scene["vehicle_centers"]):
        yaw = 0.2 * np.sin(0.3 * k + oid)
        q = yaw_q(yaw)
        t = np.asarray(cen, np.float64) - rot_z(yaw, cen) + np.array([3.0 * np.sin(0.1 * k + oid), 3.0 * np.cos(0.1 * k + oid), 0.0])
        P[oid, :4] = q
        P[oid, 4:] = t.astype(np.float32)
    return P


def median_ms(fn, n):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(np.min(ts))


def frame_rate(ctx, poses, hosts, steps, before_step=None):
    F, n = 8, 0
    ctx.wait_host(None)
    t0 = time.perf_counter()
    for k in range(steps):
        if before_step is not None:
            before_step(k)
        for b in range(2):
            h = hosts[n % len(hosts)]
            n += 1
            ctx.wait_host(h.ptr)
            ctx.simulate_batch_host_async([poses[(b * F + f) % len(poses)] for f in range(F)], h.ptr)
    ctx.wait_host(None)
    return 16 * steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 3, 4])
    ap.add_argument("--vehicles", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--refit-only", action="store_true")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    out = []
    for cid in args.configs:
        s = scenes.add_vehicles(scenes.config_scene(cid), args.vehicles)
        n_pass, n_rays = WORKLOAD[cid]
        cfg = params.kaist_preset(n_reflections=n_pass, n_samples=n_rays, ambient_noise=0)
        ctx = native.Context(0)
        t0 = time.perf_counter()
        ctx.set_mesh(s["verts"], s["faces"], s["face_object_id"])
        t_mesh = time.perf_counter() - t0
        ctx.set_materials(materials_for(s), s["object_materials"], 0)
        ctx.set_config(cfg)
        ctx.set_beam_samples(golden_beams(n_rays))
        n_obj = int(s["face_object_id"].max()) + 1
        rs = np.random.RandomState(5)
        r = {"config": cid, "triangles": int(len(s["faces"])), "vehicles": args.vehicles, "set_mesh_s": round(t_mesh, 3)}
        t0 = time.perf_counter()
        ctx.set_object_poses(jitter_poses(s, n_obj, 0, rs))          # the first dynamic call also makes the level lists
        r["first_dynamic_call_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
        k = [1]

        def move():
            ctx.set_object_poses(jitter_poses(s, n_obj, k[0], rs))
            k[0] += 1
        r["set_object_poses_ms_median_min"] = [round(x, 3) for x in median_ms(move, args.repeats)]
        verts = s["verts"]

        def update_vertices():
            # (new rest vertices: from here on every leaf takes its triangles' whole boxes -- rr_rebuild_tree restores
            # the builder's clipped ones -- so the frame-rate runs below come first)
            r["update_vertices_ms_median_min"] = [round(x, 3) for x in median_ms(lambda: ctx.update_vertices(verts), args.repeats)]
        if args.refit_only:
            update_vertices()
            out.append(r)
            print(json.dumps(r), flush=True)
            ctx.close()
            continue
        poses = scenes.trajectory(16, s["name"])
        hosts = [native.HostImages((8, cfg.n_cells, 400)) for _ in range(8)]
        ctx.set_object_poses(jitter_poses(s, n_obj, 0, rs))
        frame_rate(ctx, poses, hosts, 3)                             # warm-up: graphs captured, grids sized
        r["images_per_s_static"] = round(frame_rate(ctx, poses, hosts, args.steps), 1)
        r["images_per_s_moving"] = round(frame_rate(ctx, poses, hosts, args.steps,
                                                    lambda k: ctx.set_object_poses(jitter_poses(s, n_obj, k, rs))), 1)
        cap, rep = ctx.graph_stats()
        r["graph_captures_replays"] = [cap, rep]
        heading = rs.uniform(0, 2 * np.pi, args.vehicles)
        drive = []
        for dist in (0, 30, 60, 100, 150, 200, 300):
            ctx.set_object_poses(drive_poses(s, n_obj, dist, heading))
            now, built = ctx.tree_cost()
            frame_rate(ctx, poses, hosts, 1)
            drive.append({"m": dist, "cost_ratio": round(now / built, 4),
                          "images_per_s": round(frame_rate(ctx, poses, hosts, max(2, args.steps // 2)), 1)})
        r["drive"] = drive
        for builder in ("host", "gpu"):
            t0 = time.perf_counter()
            ctx.rebuild_tree(builder)
            r["rebuild_%s_s" % builder] = round(time.perf_counter() - t0, 3)
            now, built = ctx.tree_cost()
            frame_rate(ctx, poses, hosts, 1)
            r["after_rebuild_%s" % builder] = {"cost_ratio": round(now / built, 4),
                                               "images_per_s": round(frame_rate(ctx, poses, hosts, max(2, args.steps // 2)), 1)}
        update_vertices()
        frame_rate(ctx, poses, hosts, 1)
        r["after_update_vertices_images_per_s"] = round(frame_rate(ctx, poses, hosts, max(2, args.steps // 2)), 1)
        for h in hosts:
            h.close()
        ctx.close()
        out.append(r)
        print(json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
