#!/usr/bin/env python
"""Times the pose-graph optimiser on one MI355X on a seeded Manhattan-style trajectory: `nodes` poses one metre
apart on a street grid, a quarter turn every few steps, drifting odometry, and a closure wherever the walk comes back to a crossing it has
seen.  rr_optimize_graph_device at (iterations, cg_iterations), at (iterations, 0) and at (0, 0): device events around `reps` back-to-back
calls after a warm-up.  The time per CG step is the difference of the first two over iterations * cg_iterations, the time per outer
iteration without its CG steps the difference of the last two over iterations.  Beside them the numpy restatement (tests/graph_ref.py)
on the same graph, on this host's CPU, and whether the two agree byte for byte.  Prints one JSON line.

    python tools/probe_graph.py [--nodes 10000] [--iterations 4] [--cg 20] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import graph_ref as R  # noqa: E402
from radarays_ros_amd import native  # noqa: E402


def manhattan(n, seed, block=8, span=12):
    """-> (truth, start, fixed, edges): a walk over a street grid of `span` blocks of `block` metres, closures at crossings seen before"""
    rs = np.random.RandomState(seed)
    heading, pos, lim = 0, np.zeros(2, np.int64), span * block // 2
    dirs = np.array([[1, 0], [0, 1], [-1, 0], [0, -1]])
    xy, yaw = np.zeros((n, 2)), np.zeros(n)
    seen, ci, cj = {}, [], []
    for k in range(n):
        xy[k], yaw[k] = pos, heading * (np.pi / 2)
        key = (int(pos[0]), int(pos[1]))
        if key in seen and k - seen[key] > 2 * block:
            ci.append(seen[key]); cj.append(k)
        seen[key] = k
        if pos[0] % block == 0 and pos[1] % block == 0:                # a crossing: straight on, left or right, never out of town
            for turn in rs.permutation([0, 0, 1, -1]):
                nxt = pos + dirs[(heading + turn) % 4]
                if abs(nxt[0]) <= lim and abs(nxt[1]) <= lim:
                    heading = (heading + turn) % 4
                    break
            else:
                heading = (heading + 2) % 4
        pos = pos + dirs[heading]
    truth = R.states_of(yaw, xy[:, 0], xy[:, 1])
    a = np.arange(n - 1)
    odo = R.relative(truth[a], truth[a + 1])
    oy = np.arctan2(odo[:, 1], odo[:, 0]) + rs.normal(0, 0.002, n - 1) + 0.0005
    odo = np.stack([np.cos(oy), np.sin(oy), odo[:, 2] + rs.normal(0, 0.01, n - 1), odo[:, 3] + rs.normal(0, 0.01, n - 1)], axis=1)
    ci, cj = np.array(ci, np.int64), np.array(cj, np.int64)
    clo = R.noisy(rs, R.relative(truth[ci], truth[cj]), 0.002, 0.01)
    edges = R.edges_of(np.concatenate([a, ci]), np.concatenate([a + 1, cj]), np.concatenate([odo, clo]), 100.0, 400.0)
    start = np.zeros((n, 4))
    start[0] = truth[0]
    for k in range(n - 1):
        start[k + 1] = R.compose(start[k], odo[k])
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return truth, start, fixed, edges


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--iterations", type=int, default=4)
    ap.add_argument("--cg", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-numpy", action="store_true", help="skip the restatement (and the byte comparison)")
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    truth, start, fixed, edges = manhattan(a.nodes, a.seed)
    n, ne = len(start), len(edges)
    ctx = native.Context(0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)   # noqa: E731
    d_start, d_fixed, d_edges = up(start), up(fixed), up(edges)
    d_states = torch.empty_like(d_start)
    pb = ctx.graph_plan_bytes(n, ne)
    d_plan = torch.zeros(pb, dtype=torch.uint8, device=dev)
    cfgs = {k: native.graph_config(*k) for k in ((a.iterations, a.cg), (a.iterations, 0), (0, 0))}
    sb = max(ctx.graph_scratch_bytes(n, ne, g) for g in cfgs.values())
    d_scratch = torch.zeros(sb, dtype=torch.uint8, device=dev)
    d_recs = torch.zeros((a.iterations + 1) * 32, dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    P_ = lambda t: t.data_ptr()   # noqa: E731

    def timed(fn):
        for _ in range(2):
            fn()
        ctx.synchronize(s)
        rounds = []
        for _ in range(3):                                                # three rounds of `reps` calls: the median round is reported
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.reps):
                fn()
            e1.record(stream)
            e1.synchronize()
            rounds.append(e0.elapsed_time(e1) * 1e3 / a.reps)
        return {"median": round(sorted(rounds)[1], 1), "min": round(min(rounds), 1), "max": round(max(rounds), 1)}

    def solve(g):
        d_states.copy_(d_start)                                           # (a device copy of 32 bytes per node, inside the timing)
        ctx.optimize_graph_device(P_(d_states), P_(d_fixed), P_(d_edges), n, ne, P_(d_plan), g, P_(d_recs), P_(d_scratch), sb, None, s)

    out = {"nodes": n, "edges": ne, "closures": ne - (n - 1), "iterations": a.iterations, "cg_iterations": a.cg, "reps": a.reps, "plan_bytes": pb,
           "scratch_bytes": sb, "tiles": native.graph_tile_sizes()}
    with torch.cuda.stream(stream):
        out["plan_us"] = timed(lambda: ctx.graph_plan_device(P_(d_edges), n, ne, P_(d_plan), pb, s))
        us = {k: timed(lambda g=g: solve(g)) for k, g in cfgs.items()}
        solve(cfgs[(a.iterations, a.cg)])
    ctx.synchronize(s)
    states = d_states.cpu().numpy().view(np.float64).reshape(n, 4)
    recs = d_recs.cpu().numpy().view(native.GRAPH_REC_DTYPE)
    full, bare, none = (us[k]["median"] for k in ((a.iterations, a.cg), (a.iterations, 0), (0, 0)))
    out.update({"solve_us": us[(a.iterations, a.cg)], "solve_us_without_cg": us[(a.iterations, 0)], "solve_us_0_iterations": us[(0, 0)],
                "us_per_cg_step": round((full - bare) / max(a.iterations * a.cg, 1), 2),
                "us_per_outer_iteration_without_cg": round((bare - none) / max(a.iterations, 1), 1),
                "chi2": [float(v) for v in recs["chi2"]], "cg_stop": [int(v) for v in recs["cg_stop"]],
                "error_before_m": round(R.trajectory_error(start, truth), 4), "error_after_m": round(R.trajectory_error(states, truth), 4)})
    if not a.no_numpy:
        plan = R.Plan(edges, n)
        t0 = time.perf_counter()
        want = R.optimize(start, fixed, edges, a.iterations, a.cg, plan=plan)
        t1 = time.perf_counter()
        bare_np = R.optimize(start, fixed, edges, a.iterations, 0, plan=plan)
        t2 = time.perf_counter()
        out.update({"numpy_solve_s": round(t1 - t0, 3), "numpy_ms_per_cg_step": round(((t1 - t0) - (t2 - t1)) * 1e3 / max(a.iterations * a.cg, 1), 2),
                    "byte_equal": bool(want[0].tobytes() == states.tobytes() and want[1].tobytes() == recs.tobytes())})
        del bare_np
    print(json.dumps(out))


if __name__ == "__main__":
    main()
