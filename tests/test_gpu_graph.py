"""Pose-graph optimisation on the GPU (rr_graph.hip) against the numpy restatement of its definition (tests/graph_ref.py), byte for byte:
the states as raw f64 bits, every record and every edge flag, at the smallest graphs, at the edges of the reduction's chunks and of the
linearisation's tiles, at hub nodes on both sides of the gather's switch, with bad and flipped edges, dead blocks, a CG that stops, the
robust kernel, a reused plan, the host and the device form, two streams at once; and two seeded loops in which the optimiser must help."""
import ctypes as C

import numpy as np
import pytest

import graph_ref as R
from common import golden_beams
from radarays_ros_amd import native, params, radar

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
DEV = "cuda:0"
GUARD = 0xA5


@pytest.fixture(scope="module")
def ctx():
    return native.Context(0)


@pytest.fixture(scope="module")
def tiles():
    return native.graph_tile_sizes()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(DEV)


def plan_device(ctx, edges, n, stream=None):
    need = ctx.graph_plan_bytes(n, len(edges))
    d_edges = dev(edges) if len(edges) else None
    d_plan = torch.full((need + 64,), GUARD, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    ctx.graph_plan_device(d_edges.data_ptr() if len(edges) else None, n, len(edges), d_plan.data_ptr(), need, stream)
    torch.cuda.synchronize()
    assert (d_plan[need:].cpu().numpy() == GUARD).all()
    return d_plan[:need]


def solve_device(ctx, states, fixed, edges, d_plan=None, stream=None, **cfg):
    """rr_optimize_graph_device on guarded buffers -> (states, records, edge flags)"""
    g = native.graph_config(**cfg)
    n, ne = len(states), len(edges)
    if d_plan is None:
        d_plan = plan_device(ctx, edges, n)
    need = ctx.graph_scratch_bytes(n, ne, g)
    d_st = torch.cat([dev(np.asarray(states, np.float64)), torch.full((64,), GUARD, dtype=torch.uint8, device=DEV)])
    d_fx, d_edges = dev(np.asarray(fixed, np.uint8)), dev(edges) if ne else None
    d_rec = torch.full(((g.iterations + 1) * 32 + 64,), GUARD, dtype=torch.uint8, device=DEV)
    d_flag = torch.full((ne + 64,), GUARD, dtype=torch.uint8, device=DEV)
    d_scr = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device=DEV)     # (the scratch's contents before the call do not matter)
    torch.cuda.synchronize()
    ctx.optimize_graph_device(d_st.data_ptr(), d_fx.data_ptr(), d_edges.data_ptr() if ne else None, n, ne, d_plan.data_ptr(), g, d_rec.data_ptr(),
                              d_scr.data_ptr(), need, d_flag.data_ptr(), stream)
    torch.cuda.synchronize()
    st, rec, fl = d_st.cpu().numpy(), d_rec.cpu().numpy(), d_flag.cpu().numpy()
    assert (st[n * 32:] == GUARD).all() and (rec[(g.iterations + 1) * 32:] == GUARD).all() and (fl[ne:] == GUARD).all()
    assert (d_scr[need:].cpu().numpy() == 0x5A).all()
    return st[:n * 32].view(np.float64).reshape(n, 4).copy(), rec[:(g.iterations + 1) * 32].view(native.GRAPH_REC_DTYPE).copy(), fl[:ne].copy()


def same(got, want):
    """states as raw bits, records and flags whole"""
    assert got[1].tobytes() == want[1].tobytes(), (got[1], want[1])
    assert got[2].tobytes() == want[2].tobytes()
    assert got[0].tobytes() == want[0].tobytes(), np.abs(got[0] - want[0]).max()


def check(ctx, states, fixed, edges, **cfg):
    want = R.optimize(states, fixed, edges, **cfg)
    got = solve_device(ctx, states, fixed, edges, **cfg)
    same(got, want)
    return got


CFG = dict(iterations=3, cg_iterations=12, lam=0.0, robust_k=0.0)


def test_the_records_are_the_restatements_dtype():
    assert native.GRAPH_EDGE_DTYPE == R.EDGE_DTYPE and native.GRAPH_REC_DTYPE == R.REC_DTYPE
    assert (native.GRAPH_EDGE_FLIPPED, native.GRAPH_EDGE_BAD) == (R.FLIPPED, R.BAD) and native.graph_tile_sizes() == (R.CHUNK, R.CHUNK)


def test_the_plan_lists_every_nodes_edges_in_ascending_index(ctx):
    start, _, edges = R.random_graph(11, 300, 1500)
    edges["i"][:200] = 7                                             # a hub, filled by many workgroups at once
    edges["j"][:200] = np.arange(8, 208)
    edges["j"][300] = 4000; edges["i"][301] = edges["j"][301]        # bad endpoints are left out
    plan = plan_device(ctx, edges, 300).cpu().numpy()
    want = R.Plan(edges, 300)
    words = plan.view(np.uint32)
    assert words[1] == 300 and words[2] == len(edges)
    assert np.array_equal(words[4:4 + 301], want.offsets) and np.array_equal(words[4 + 304:4 + 304 + len(want.lists)], want.lists)
    assert plan.tobytes() == plan_device(ctx, edges[:], 300).cpu().numpy().tobytes() == ctx.graph_plan(edges, 300).tobytes()


def test_the_smallest_graphs(ctx):
    one = R.states_of([0.3], [1.0], [2.0])
    for fixed in ([0], [1]):
        got = check(ctx, one, fixed, np.zeros(0, R.EDGE_DTYPE), **CFG)
        assert got[0].tobytes() == one.tobytes() and got[1]["n_dead"][0] == 1 - fixed[0] and got[1]["cg_stop"][0] == 0
    two = R.states_of([0.1, 0.5], [0.0, 1.2], [0.0, -0.1])
    z = R.states_of([0.3], [1.0], [0.1])
    for i, j in ((0, 1), (1, 0)):
        for fixed in ([1, 0], [0, 1]):
            got = check(ctx, two, fixed, R.edges_of([i], [j], z, 50.0, 80.0), **CFG)
            assert got[1]["chi2"][-1] < 1e-6 * got[1]["chi2"][0]          # one edge, one free node: it can be met
    dup = R.edges_of([0, 0, 1, 0], [1, 1, 0, 1], np.concatenate([z, z, R.relative(z, R.states_of([0.0], [0.0], [0.0])), z]), 50.0, 80.0)
    check(ctx, two, [1, 0], dup, **CFG)


def test_an_isolated_node_is_a_dead_block_without_lambda_and_stays_put_with_it(ctx):
    start, fixed, edges = R.random_graph(5, 6, 8)
    keep = (edges["i"] != 5) & (edges["j"] != 5)
    edges = edges[keep]
    got = check(ctx, start, fixed, edges, **CFG)
    assert got[1]["n_dead"][:-1].tolist() == [1, 1, 1] and got[1]["n_dead"][-1] == 0 and got[0][5].tobytes() == start[5].tobytes()
    got = check(ctx, start, fixed, edges, **dict(CFG, lam=0.5))
    assert got[1]["n_dead"].tolist() == [0, 0, 0, 0] and got[0][5].tobytes() == start[5].tobytes()
    assert got[0][4].tobytes() != start[4].tobytes()


@pytest.mark.parametrize("offset", [-1, 0, 1, "2c+1"])
def test_node_counts_at_the_reduction_chunks_edges(ctx, tiles, offset):
    n = 2 * tiles[0] + 1 if offset == "2c+1" else tiles[0] + offset
    start, fixed, edges = R.random_graph(20, n, n + 40)
    check(ctx, start, fixed, edges, **CFG)


@pytest.mark.parametrize("offset", [-1, 0, 1, "2c+1"])
def test_edge_counts_at_the_linearisation_tiles_edges(ctx, tiles, offset):
    ne = 2 * tiles[1] + 1 if offset == "2c+1" else tiles[1] + offset
    start, fixed, edges = R.random_graph(21, 100, ne)
    got = check(ctx, start, fixed, edges, **dict(CFG, robust_k=2.0))
    assert got[1]["n_used"].tolist() == [ne] * 4


@pytest.mark.parametrize("degree", [1, 63, 64, 65, 200])
def test_a_hub_gathers_in_ascending_edge_index(ctx, degree):
    """Node 3 has `degree` edges whose weights span twenty orders of magnitude, so the f64 sum of its block depends on the order: the bytes
    are the restatement's, and differ from a solve with the hub's edges renumbered."""
    n = degree + 8
    start, fixed, edges = R.random_graph(30 + degree, n, n - 1)
    others = np.array([k for k in range(n) if k != 3][:degree])
    rs = np.random.RandomState(degree)
    z = R.noisy(rs, R.relative(start[np.full(degree, 3)], start[others]), 0.02, 0.05)
    flip = rs.rand(degree) < 0.5                                       # the hub on either side of its edges
    hub = R.edges_of(np.where(flip, others, 3), np.where(flip, 3, others), np.where(flip[:, None], R.relative(z, R.states_of([0.0], [0.0], [0.0]).repeat(degree, 0)), z),
                     10.0 ** rs.uniform(-8, 8, degree), 10.0 ** rs.uniform(-8, 8, degree))
    edges = np.concatenate([edges[:5], hub, edges[5:]])
    got = check(ctx, start, fixed, edges, **dict(CFG, lam=1e-3))
    if degree > 1:
        mixed = edges.copy()
        mixed[5:5 + degree] = hub[::-1]
        assert R.optimize(start, fixed, mixed, **dict(CFG, lam=1e-3))[0].tobytes() != got[0].tobytes()


def test_no_iterations_and_no_cg_steps_leave_the_states_bytes(ctx):
    start, fixed, edges = R.random_graph(40, 50, 90)
    start[7, :2] *= 1.0 + 1e-9                                          # a state that renormalisation would change
    got = check(ctx, start, fixed, edges, iterations=0, cg_iterations=5)
    assert got[0].tobytes() == start.tobytes() and len(got[1]) == 1 and got[1]["chi2"][0] == R.cost(start, edges)
    got = check(ctx, start, fixed, edges, iterations=2, cg_iterations=0)
    assert got[0].tobytes() == start.tobytes() and got[1]["chi2"].tolist() == [R.cost(start, edges)] * 3 and got[1]["cg_stop"].tolist() == [-1] * 3


def test_bad_and_flipped_edges_are_flagged_counted_and_left_out(ctx):
    start, fixed, edges = R.random_graph(41, 40, 70)
    sick = edges[:8].copy()
    sick["i"][0] = sick["j"][0]
    sick["i"][1] = 40
    sick["j"][2] = 0xFFFFFFFF
    sick["tx"][3] = np.nan
    sick["c"][4] = np.inf
    sick["w_t"][5] = np.inf
    sick["w_r"][6] = -1.0
    far = R.relative(start[sick["i"][7:8]], start[sick["j"][7:8]])      # the turn between two nodes as it stands, plus pi; the two are
    sick["c"][7], sick["s"][7] = -far[0, 0], -far[0, 1]                 # fixed, so the edge stays flipped at every linearisation
    fixed[[sick["i"][7], sick["j"][7]]] = 1
    where = [3, 9, 20, 21, 35, 50, 60, 77]
    mixed = np.insert(edges, [w - k for k, w in enumerate(where)], sick)
    assert all(mixed[w].tobytes() == sick[k].tobytes() for k, w in enumerate(where))
    got = check(ctx, start, fixed, mixed, **CFG)
    flags = np.zeros(len(mixed), np.uint8)
    flags[where[:7]] = R.BAD
    flags[where[7]] = R.FLIPPED
    assert np.array_equal(got[2], flags)
    assert got[1]["n_bad"].tolist() == [7] * 4 and got[1]["n_flipped"].tolist() == [1] * 4 and got[1]["n_used"].tolist() == [70] * 4
    # only omitted terms differ: the states' bits are those of the graph without the flagged edges; chi2 is reduced over the edge INDEX, so
    # with the flagged edges behind the others it is the same bits too, and with them in between the same sum in another order
    clean = R.optimize(start, fixed, edges, **CFG)
    assert clean[0].tobytes() == got[0].tobytes() and np.allclose(clean[1]["chi2"], got[1]["chi2"], rtol=1e-13, atol=0)
    behind = check(ctx, start, fixed, np.concatenate([edges, sick]), **CFG)
    assert clean[0].tobytes() == behind[0].tobytes() and np.array_equal(clean[1]["chi2"], behind[1]["chi2"])


def test_all_nodes_fixed_stops_the_cg_at_its_first_step(ctx):
    start, _, edges = R.random_graph(42, 30, 50)
    got = check(ctx, start, np.ones(30, np.uint8), edges, **CFG)
    assert got[1]["cg_stop"].tolist() == [0, 0, 0, -1] and got[0].tobytes() == start.tobytes() and got[1]["chi2"][0] > 0


def test_robust_weights(ctx):
    start, fixed, edges = R.random_graph(43, 80, 160)
    plain = check(ctx, start, fixed, edges, **CFG)
    assert R.optimize(start, fixed, edges, iterations=3, cg_iterations=12)[0].tobytes() == plain[0].tobytes()
    robust = check(ctx, start, fixed, edges, **dict(CFG, robust_k=1.5))
    assert robust[0].tobytes() != plain[0].tobytes()


OUTLIER = dict(per_side=4, closures=((0, -1), (2, 10), (5, 13)), outliers=((3, 11, 3.0, -2.0),))


def test_one_gross_outlier_bends_the_loop_less_with_the_kernel_on(ctx):
    """A 16-node loop with three true closures and one closure that is 3.6 m wrong.  In the restatement, here on the CPU, the loop ends
    0.4765 m from the truth without the kernel and 0.0295 m with robust_k = 1: the bound between them is 0.1 m."""
    truth, start, fixed, edges = R.loop_graph(9, **OUTLIER)
    off = check(ctx, start, fixed, edges, iterations=12, cg_iterations=45)
    on = check(ctx, start, fixed, edges, iterations=12, cg_iterations=45, robust_k=1.0)
    print("outlier loop: %.4f m off, %.4f m on" % (R.trajectory_error(off[0], truth), R.trajectory_error(on[0], truth)))
    assert R.trajectory_error(on[0], truth) < 0.1 < R.trajectory_error(off[0], truth)


def test_a_closed_loop_is_pulled_together(ctx):
    """64 poses round a square, drifting odometry, one true closure: 1.484 m from the truth before, 0.282 m after (restatement, CPU)."""
    truth, start, fixed, edges = R.loop_graph(5)
    got = check(ctx, start, fixed, edges, iterations=8, cg_iterations=60)
    before, after = R.trajectory_error(start, truth), R.trajectory_error(got[0], truth)
    print("closed loop: %.4f m before, %.4f m after, chi2 %s" % (before, after, got[1]["chi2"]))
    assert after < 0.5 * before and np.all(np.diff(got[1]["chi2"]) <= 0)


def test_same_bytes_twice_from_both_forms_and_from_a_reused_plan(ctx):
    start, fixed, edges = R.random_graph(44, 300, 520)
    d_plan = plan_device(ctx, edges, 300)
    first = solve_device(ctx, start, fixed, edges, d_plan, **CFG)
    same(solve_device(ctx, start, fixed, edges, d_plan, **CFG), first)
    plan = ctx.graph_plan(edges, 300)
    host = ctx.optimize_graph(start, fixed, edges, CFG, plan=plan, want_flags=True)
    same(host, first)
    same(ctx.optimize_graph(start, fixed, edges, CFG, want_flags=True), first)
    moved = edges.copy()                                                # new measurements between the same endpoints: the plan serves again
    moved["tx"] += 0.05
    moved["w_t"] *= 2.0
    again = solve_device(ctx, start, fixed, moved, d_plan, **CFG)
    same(again, R.optimize(start, fixed, moved, **CFG))
    assert again[0].tobytes() != first[0].tobytes()


def test_two_streams_solve_different_graphs_at_once_beside_a_batch_in_flight():
    import icp_ref as P
    s, cfg = P.loop_scene(), P.loop_cfg()
    c = native.Context(0)
    c.set_mesh(s["verts"], s["faces"], s["face_object_id"])
    c.set_materials(params.kaist_materials(), s["object_materials"], 0)
    c.set_config(cfg, P.LOOP_ANGLES)
    c.set_beam_samples(golden_beams(P.LOOP_SAMPLES))
    poses = np.stack([P.loop_pose((0.1 * k, 0.05 * k, 0.01 * k)) for k in range(8)])
    imgs = torch.zeros((8, cfg.n_cells, P.LOOP_ANGLES), dtype=torch.uint8, device=DEV)
    g = native.graph_config(**CFG)
    work = []
    for seed, n, ne in ((51, 700, 1300), (52, 513, 900)):
        start, fixed, edges = R.random_graph(seed, n, ne)
        b = dict(st=dev(start), fx=dev(fixed), ed=dev(edges), plan=plan_device(c, edges, n), rec=torch.zeros(4 * 32, dtype=torch.uint8, device=DEV),
                 scr=torch.zeros(c.graph_scratch_bytes(n, ne, g), dtype=torch.uint8, device=DEV))
        work.append((b, start, n, ne, torch.cuda.Stream(device=DEV), R.optimize(start, fixed, edges, **CFG)))
    torch.cuda.synchronize()

    def enqueue(b, n, ne, stream):
        c.optimize_graph_device(b["st"].data_ptr(), b["fx"].data_ptr(), b["ed"].data_ptr(), n, ne, b["plan"].data_ptr(), g, b["rec"].data_ptr(),
                                b["scr"].data_ptr(), b["scr"].numel(), None, stream)

    c.simulate_batch_device(poses, imgs.data_ptr(), None)             # a batch in flight on the context's stream
    for b, _, n, ne, s_, _ in work:
        enqueue(b, n, ne, s_.cuda_stream)
    torch.cuda.synchronize()
    c.synchronize()
    busy = imgs.cpu().numpy().copy()
    for b, _, _, _, _, want in work:
        assert b["st"].cpu().numpy().tobytes() == want[0].tobytes() and b["rec"].cpu().numpy().tobytes() == want[1].tobytes()
    imgs.zero_()
    torch.cuda.synchronize()
    c.simulate_batch_device(poses, imgs.data_ptr(), None)
    c.synchronize()
    assert np.array_equal(imgs.cpu().numpy(), busy) and busy.any()    # ... and the batch beside them was not disturbed


def test_every_refusal_leaves_its_outputs_untouched(ctx):
    L = ctx._L
    start, fixed, edges = R.random_graph(45, 20, 30)
    g = native.graph_config(**CFG)
    pb, sb = ctx.graph_plan_bytes(20, 30), ctx.graph_scratch_bytes(20, 30, g)
    buf = torch.full((pb + sb + 8192,), GUARD, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    assert p % 16 == 0
    d_edges, d_st, d_fx = dev(edges), dev(start), dev(fixed)
    e, s, f = d_edges.data_ptr(), d_st.data_ptr(), d_fx.data_ptr()
    bad_plan = [(None, 20, 30, p, pb), (e, 20, 30, None, pb), (e, 0, 30, p, pb), (e, (1 << 20) + 1, 30, p, pb), (e, 20, -1, p, pb),
                (e, 20, (1 << 22) + 1, p, pb), (e, 20, 30, p, pb - 1), (e + 8, 20, 30, p, pb), (e, 20, 30, p + 4, pb)]
    for a in bad_plan:
        assert L.rr_graph_plan_device(ctx._h, *a, None) == -3, a
        assert b"rr_graph_plan_device" in L.rr_last_error(ctx._h)
    assert L.rr_graph_plan_device(None, e, 20, 30, p, pb, None) == -1
    assert L.rr_graph_plan(ctx._h, None, 20, 30, p, pb) == -3 and L.rr_graph_plan(None, None, 20, 30, p, pb) == -1
    ctx.graph_plan_device(e, 20, 30, p, pb)
    torch.cuda.synchronize()
    plan, rec, scr = p, p + pb + 1024, p + pb + 2048
    assert plan % 16 == 0 and rec % 16 == 0 and scr % 16 == 0
    before = buf.cpu().numpy().copy()

    def cfg_with(**kw):
        c = native.graph_config(**CFG)
        for k, v in kw.items():
            if k == "reserved_":
                c.reserved_[1] = v
            else:
                setattr(c, k, v)
        return c

    ok = dict(s=s, f=f, e=e, n=20, ne=30, plan=plan, g=g, rec=rec, fl=None, scr=scr, sb=sb)
    wrong = [dict(s=None), dict(f=None), dict(e=None), dict(plan=None), dict(g=None), dict(rec=None), dict(scr=None), dict(n=0), dict(n=(1 << 20) + 1),
             dict(ne=-1), dict(ne=(1 << 22) + 1), dict(sb=sb - 1), dict(s=s + 8), dict(e=e + 8), dict(plan=plan + 8), dict(rec=rec + 8), dict(scr=scr + 8),
             dict(g=cfg_with(iterations=257)), dict(g=cfg_with(iterations=-1)), dict(g=cfg_with(cg_iterations=1025)), dict(g=cfg_with(cg_iterations=-1)),
             dict(g=cfg_with(**{"lambda": -1.0})), dict(g=cfg_with(**{"lambda": float("nan")})), dict(g=cfg_with(**{"lambda": float("inf")})),
             dict(g=cfg_with(robust_k=-0.5)), dict(g=cfg_with(robust_k=float("nan"))), dict(g=cfg_with(reserved_=1))]
    for w in wrong:
        a = dict(ok, **w)
        rc = L.rr_optimize_graph_device(ctx._h, a["s"], a["f"], a["e"], a["n"], a["ne"], a["plan"], C.byref(a["g"]) if a["g"] is not None else None, a["rec"],
                                        a["fl"], a["scr"], a["sb"], None)
        assert rc == -3 and b"rr_optimize_graph_device" in L.rr_last_error(ctx._h), w
    assert L.rr_optimize_graph_device(None, s, f, e, 20, 30, plan, C.byref(g), rec, None, scr, sb, None) == -1
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), before) and d_st.cpu().numpy().tobytes() == start.tobytes()
    # the host form: its outputs are the caller's arrays
    hs, hr = start.copy(), np.full(4, 7, native.GRAPH_REC_DTYPE)
    hp = np.zeros(pb, np.uint8)
    assert L.rr_optimize_graph(ctx._h, hs.ctypes.data, fixed.ctypes.data, edges.ctypes.data, 20, 30, hp.ctypes.data, C.byref(cfg_with(iterations=300)),
                               hr.ctypes.data, None) == -3
    assert L.rr_optimize_graph(ctx._h, hs.ctypes.data, None, edges.ctypes.data, 20, 30, hp.ctypes.data, C.byref(g), hr.ctypes.data, None) == -3
    assert hs.tobytes() == start.tobytes() and (hr["n_used"] == 7).all()
    for bad in (dict(iterations=-1), dict(cg_iterations=2000), dict(lam=-1.0), dict(robust_k=float("inf")), dict(lam="x")):
        with pytest.raises(ValueError):
            native.graph_config(**bad)
    with pytest.raises(ValueError):
        ctx.optimize_graph(start[:, :3], fixed, edges, CFG)
    with pytest.raises(ValueError):
        ctx.optimize_graph(start, fixed[:5], edges, CFG)
    with pytest.raises(ValueError):
        ctx.optimize_graph(start, fixed, edges, CFG, plan=np.zeros(8, np.uint8))
    assert ctx.graph_plan_bytes(20, 30) == pb and L.rr_graph_plan_bytes(0, 1) == 0 and L.rr_graph_scratch_bytes(20, 30, None) == 0


def test_the_python_facade_gives_the_ctypes_paths_bytes(ctx):
    truth, start, fixed, edges = R.loop_graph(6, per_side=5)
    want = ctx.optimize_graph(start, fixed, edges, CFG)
    r = radar.RadarHIP.__new__(radar.RadarHIP)                         # (the method needs the context alone)
    r._ctx = ctx
    states, recs = r.optimizePoseGraph(start, fixed, edges, **CFG)
    assert states.tobytes() == want[0].tobytes() and recs.tobytes() == want[1].tobytes()
    same((states, recs, np.zeros(0)), R.optimize(start, fixed, edges, **CFG)[:2] + (np.zeros(0),))
    packed = native.graph_edges(edges["i"], edges["j"], np.stack([edges[k] for k in ("c", "s", "tx", "ty")], 1), edges["w_t"], edges["w_r"])
    assert packed.tobytes() == edges.tobytes()
