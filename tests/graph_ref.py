"""The pose-graph optimiser of include/radarays_mi355.h ("pose-graph optimisation") restated in numpy: f64, + - * / sqrt as written, every
sum in the header's order with explicit adds (never np.sum or np.dot), so that rr_optimize_graph can be held to it byte for byte.

NODES are float64 [N][4] = (c, s, tx, ty) with a fixed byte each, EDGES native.GRAPH_EDGE_DTYPE records.  Names follow the header:
  linearize   an edge's residual (etx, ety, er), its flag, chi and terms
  Plan        every node's incident edges in ascending edge index (edges with a bad endpoint left out)
  list_sum    the LIST SUM: one after the other up to 64 entries, 64 strided lane sums and a halving beyond
  reduce      the REDUCTION: a halving tree inside chunks of 256, the partials strided over 256 slots and halved again
  optimize    the outer iterations: linearise, gather, preconditioned CG of a fixed step count, update; one record each and a last one
"""
import numpy as np

CHUNK, HUB = 256, 64
FLIPPED, BAD = 1, 2
FLIP_DEN = 2.0 ** -20
EDGE_DTYPE = np.dtype([("i", "<u4"), ("j", "<u4"), ("c", "<f8"), ("s", "<f8"), ("tx", "<f8"), ("ty", "<f8"), ("w_t", "<f4"), ("w_r", "<f4")])
REC_DTYPE = np.dtype([("chi2", "<f8"), ("n_used", "<u4"), ("n_flipped", "<u4"), ("n_bad", "<u4"), ("n_dead", "<u4"), ("cg_stop", "<i4"),
                      ("reserved_", "<u4")])


# ---- the reduction ---------------------------------------------------------------------------------------------------------------------
def _halve(v):
    """v [..][256] -> [..]: for h = 128 .. 1: v[t] = v[t] + v[t + h], t < h"""
    v = v.copy()
    h = v.shape[-1] // 2
    while h:
        v[..., :h] = v[..., :h] + v[..., h:2 * h]
        h //= 2
    return v[..., 0]


def chunk_partials(vals):
    """the partial of every chunk of 256 consecutive values, the last chunk padded with 0.0"""
    m = (len(vals) + CHUNK - 1) // CHUNK
    v = np.zeros(m * CHUNK)
    v[:len(vals)] = vals
    return _halve(v.reshape(m, CHUNK)).reshape(m)


def combine(part):
    """s[t] = P[t] + P[t + 256] + .. one after the other from 0.0, then the halving over s"""
    rows = (len(part) + CHUNK - 1) // CHUNK
    pad = np.zeros(rows * CHUNK)
    pad[:len(part)] = part
    s = np.zeros(CHUNK)
    for k in range(rows):
        s = s + pad[k * CHUNK:(k + 1) * CHUNK]          # (a slot past the end adds 0.0 to a sum that is never -0.0: no change)
    return float(_halve(s))


def reduce(vals):
    return combine(chunk_partials(np.asarray(vals, np.float64)))


def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
class Plan:
    """offsets [N + 1] and lists [offsets[N]] as rr_graph_plan gives them, and what the list sum needs of them"""

    def __init__(self, edges, n_nodes):
        i, j = edges["i"].astype(np.int64), edges["j"].astype(np.int64)
        ok = np.nonzero((i != j) & (i < n_nodes) & (j < n_nodes))[0]
        node, edge = np.concatenate([i[ok], j[ok]]), np.concatenate([ok, ok])
        order = np.lexsort((edge, node))
        self.n_nodes = n_nodes
        self.node, self.lists = node[order], edge[order]
        self.deg = np.bincount(self.node, minlength=n_nodes).astype(np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.deg)])
        pos = np.arange(len(self.lists)) - self.offsets[self.node]
        short = self.deg[self.node] <= HUB
        top = int(self.deg[self.deg <= HUB].max(initial=0))
        self.by_pos = [np.nonzero(short & (pos == k))[0] for k in range(top)]
        self.hubs = np.nonzero(self.deg > HUB)[0]


def list_sum(C, plan):
    """C [entries][K]: the term of every list entry (0.0 for a flagged edge: adding it changes nothing) -> [N][K]"""
    out = np.zeros((plan.n_nodes, C.shape[1]))
    for sel in plan.by_pos:
        n = plan.node[sel]
        out[n] = out[n] + C[sel]
    for n in plan.hubs:
        b, L = int(plan.offsets[n]), int(plan.deg[n])
        rows = (L + 63) // 64
        pad = np.zeros((rows * 64, C.shape[1]))
        pad[:L] = C[b:b + L]
        lanes = np.zeros((64, C.shape[1]))
        for r in range(rows):
            lanes = lanes + pad[r * 64:(r + 1) * 64]
        h = 32
        while h:
            lanes[:h] = lanes[:h] + lanes[h:2 * h]
            h //= 2
        out[n] = lanes[0]
    return out


# ---- an edge ---------------------------------------------------------------------------------------------------------------------------
def linearize(states, edges, robust_k=0.0):
    """-> dict of float64 [E] planes ci si ux uy kk wt wr etx ety er chi (0.0 where flagged), and flags uint8 [E]"""
    N, E = len(states), len(edges)
    i, j = edges["i"].astype(np.int64), edges["j"].astype(np.int64)
    wt0, wr0 = edges["w_t"].astype(np.float64), edges["w_r"].astype(np.float64)
    flags = np.zeros(E, np.uint8)
    fin = np.isfinite(edges["c"]) & np.isfinite(edges["s"]) & np.isfinite(edges["tx"]) & np.isfinite(edges["ty"]) & np.isfinite(wt0) & np.isfinite(wr0)
    with np.errstate(invalid="ignore"):
        bad = ~((i != j) & (i < N) & (j < N)) | ~fin | ~(wt0 >= 0.0) | ~(wr0 >= 0.0)
    flags[bad] = BAD
    T = {k: np.zeros(E) for k in ("ci", "si", "ux", "uy", "kk", "wt", "wr", "etx", "ety", "er", "chi")}
    a_ = np.nonzero(~bad)[0]
    k2 = robust_k * robust_k
    with np.errstate(all="ignore"):
        si_, sj_ = states[i[a_]], states[j[a_]]
        ci, si, cj, sj = si_[:, 0], si_[:, 1], sj_[:, 0], sj_[:, 1]
        dx, dy = sj_[:, 2] - si_[:, 2], sj_[:, 3] - si_[:, 3]
        ux, uy = ci * dx + si * dy, ci * dy - si * dx
        etx, ety = ux - edges["tx"][a_], uy - edges["ty"][a_]
        a, b = ci * cj + si * sj, ci * sj - si * cj
        zc, zs = edges["c"][a_], edges["s"][a_]
        rc, rs = zc * a + zs * b, zc * b - zs * a
        den = 1.0 + rc
        flipped = ~(den >= FLIP_DEN)
        er = (2.0 * rs) / den
        wt, wr = wt0[a_], wr0[a_]
        chi = wt * (etx * etx + ety * ety) + wr * (er * er)
        nonfin = ~flipped & ~np.isfinite(chi)
        if k2 > 0.0:
            sc = 1.0 / (1.0 + chi / k2)
            wt, wr = wt * sc, wr * sc
        kk = 1.0 + (er * er) / 4.0
    flags[a_[flipped]] = FLIPPED
    flags[a_[nonfin]] = BAD
    use = ~flipped & ~nonfin
    u = a_[use]
    for name, v in (("ci", ci), ("si", si), ("ux", ux), ("uy", uy), ("kk", kk), ("wt", wt), ("wr", wr), ("etx", etx), ("ety", ety), ("er", er), ("chi", chi)):
        T[name][u] = v[use]
    return T, flags


def cost(states, edges):
    """chi2 of the header over the unflagged edges, in the reduction's order"""
    T, _ = linearize(np.asarray(states, np.float64), edges)
    return reduce(T["chi"])


def _entry_terms(T, flags, edges, plan):
    """the planes of T per list entry, whether the entry's node is the edge's i, and whether the edge is in use"""
    e = plan.lists
    t = {k: v[e] for k, v in T.items()}
    return t, edges["i"][e].astype(np.int64) == plan.node, flags[e] == 0


def gather(T, flags, edges, plan):
    """-> S [N][7] = H00 H01 H02 H11 g0 g1 g2 per node"""
    t, as_i, use = _entry_terms(T, flags, edges, plan)
    ci, si, ux, uy, kk, wt, wr, etx, ety, er = (t[k] for k in ("ci", "si", "ux", "uy", "kk", "wt", "wr", "etx", "ety", "er"))
    nn = ci * ci + si * si
    Ci = np.stack([wt * (uy * uy + ux * ux) + wr * (kk * kk), -(wt * (uy * ci + ux * si)), wt * (ux * ci - uy * si), wt * nn,
                   wt * (uy * etx - ux * ety) - wr * (kk * er), wt * (si * ety - ci * etx), -(wt * (si * etx + ci * ety))], axis=1)
    zero = np.zeros_like(ci)
    Cj = np.stack([wr * (kk * kk), zero, zero, wt * nn, wr * (kk * er), wt * (ci * etx - si * ety), wt * (si * etx + ci * ety)], axis=1)
    C = np.where(as_i[:, None], Ci, Cj)
    C[~use] = 0.0
    return list_sum(C, plan)


def gradient(states, fixed, edges):
    """g = J^T W e of the header's gather, [N][3] = (d/dth, d/dx, d/dy) per node; fixed nodes included (the caller masks them)"""
    states = np.asarray(states, np.float64)
    T, flags = linearize(states, edges)
    return gather(T, flags, edges, Plan(edges, len(states)))[:, 4:7]


class Ldl:
    """the block factors of every node at once; ok: all three pivots > 0"""

    def __init__(self, S, lam):
        with np.errstate(all="ignore"):
            d = S[:, 3] + lam
            self.d0 = S[:, 0] + lam
            self.l10, self.l20 = S[:, 1] / self.d0, S[:, 2] / self.d0
            self.d1 = d - self.l10 * S[:, 1]
            m21 = 0.0 - self.l20 * S[:, 1]
            self.l21 = m21 / self.d1
            self.d2 = (d - self.l20 * S[:, 2]) - self.l21 * m21
            self.ok = (self.d0 > 0.0) & (self.d1 > 0.0) & (self.d2 > 0.0)

    def solve(self, v):
        with np.errstate(all="ignore"):
            z0 = v[:, 0]
            z1 = v[:, 1] - self.l10 * z0
            z2 = (v[:, 2] - self.l20 * z0) - self.l21 * z1
            x2 = z2 / self.d2
            x1 = z1 / self.d1 - self.l21 * x2
            x0 = (z0 / self.d0 - self.l10 * x1) - self.l20 * x2
        return np.stack([x0, x1, x2], axis=1)


def product(p, T, flags, edges, plan):
    """the list sums of the product terms: [N][3] (lambda * p is added by the caller)"""
    t, as_i, use = _entry_terms(T, flags, edges, plan)
    ci, si, ux, uy, kk, wt, wr = (t[k] for k in ("ci", "si", "ux", "uy", "kk", "wt", "wr"))
    # (a flagged edge's endpoints may be anything: node 0 stands in, its term is zeroed below)
    ei = np.where(use, edges["i"][plan.lists].astype(np.int64), 0)
    ej = np.where(use, edges["j"][plan.lists].astype(np.int64), 0)
    pi, pj = p[ei], p[ej]
    with np.errstate(all="ignore"):
        v0 = ((uy * pi[:, 0] - ci * pi[:, 1]) - si * pi[:, 2]) + (ci * pj[:, 1] + si * pj[:, 2])
        v1 = ((si * pi[:, 1] - ux * pi[:, 0]) - ci * pi[:, 2]) + (ci * pj[:, 2] - si * pj[:, 1])
        v2 = kk * (pj[:, 0] - pi[:, 0])
        y0, y1, y2 = wt * v0, wt * v1, wr * v2
        Ci = np.stack([(uy * y0 - ux * y1) - kk * y2, si * y1 - ci * y0, -(si * y0 + ci * y1)], axis=1)
        Cj = np.stack([kk * y2, ci * y0 - si * y1, si * y0 + ci * y1], axis=1)
    C = np.where(as_i[:, None], Ci, Cj)
    C[~use] = 0.0
    with np.errstate(all="ignore"):
        return list_sum(C, plan)


def _finite_pos(v):
    return v > 0.0 and v < np.inf


def optimize(states, fixed, edges, iterations=10, cg_iterations=50, lam=0.0, robust_k=0.0, plan=None):
    """-> (states [N][4], REC_DTYPE [iterations + 1], edge flags uint8 [E]) as rr_optimize_graph gives them"""
    x_ = np.array(states, np.float64, order="C")
    N = len(x_)
    free = np.asarray(fixed).astype(bool) == 0
    plan = plan or Plan(edges, N)
    recs = np.zeros(iterations + 1, REC_DTYPE)

    def record(rec, T, flags):
        rec["chi2"] = reduce(T["chi"])
        rec["n_used"], rec["n_flipped"], rec["n_bad"] = np.sum(flags == 0), np.sum(flags == FLIPPED), np.sum(flags == BAD)
        rec["cg_stop"] = -1

    for it in range(iterations):
        T, flags = linearize(x_, edges, robust_k)
        record(recs[it], T, flags)
        S = gather(T, flags, edges, plan)
        f = Ldl(S, lam)
        active = free & f.ok
        recs[it]["n_dead"] = np.sum(free & ~f.ok)
        a3 = active[:, None]
        r = np.where(a3, -S[:, 4:7], 0.0)
        z = np.where(a3, f.solve(r), 0.0)
        x = np.zeros((N, 3))
        rz_part = chunk_partials(np.where(active, dot3(r, z), 0.0))
        p, rz_before = None, None
        for k in range(cg_iterations):
            rz = combine(rz_part)
            with np.errstate(all="ignore"):
                p = z if k == 0 else z + (rz / rz_before) * p
                q = product(p, T, flags, edges, plan)
                q = np.where(a3, q + lam * p, 0.0)
                pAp = combine(chunk_partials(np.where(active, dot3(p, q), 0.0)))
            if not (_finite_pos(pAp) and _finite_pos(rz)):
                recs[it]["cg_stop"] = k
                break
            with np.errstate(all="ignore"):
                alpha = rz / pAp
                x = np.where(a3, x + alpha * p, x)
                r = np.where(a3, r - alpha * q, r)
                z = np.where(a3, f.solve(r), z)
                rz_part = chunk_partials(np.where(active, dot3(r, z), 0.0))
            rz_before = rz
        move = active & ((x[:, 0] != 0.0) | (x[:, 1] != 0.0) | (x[:, 2] != 0.0))
        with np.errstate(all="ignore"):
            u = x[:, 0] / 2.0
            dc, ds = (1.0 - u * u) / (1.0 + u * u), (2.0 * u) / (1.0 + u * u)
            c1, s1 = x_[:, 0] * dc - x_[:, 1] * ds, x_[:, 1] * dc + x_[:, 0] * ds
            nrm = np.sqrt(c1 * c1 + s1 * s1)
            new = np.stack([c1 / nrm, s1 / nrm, x_[:, 2] + x[:, 1], x_[:, 3] + x[:, 2]], axis=1)
        x_ = np.where(move[:, None], new, x_)
    T, flags = linearize(x_, edges, robust_k)
    record(recs[iterations], T, flags)
    return x_, recs, flags


# ---- seeded graphs the tests and the probe share ---------------------------------------------------------------------------------------
def edges_of(i, j, z, w_t=1.0, w_r=1.0):
    e = np.zeros(len(i), EDGE_DTYPE)
    e["i"], e["j"] = i, j
    z = np.asarray(z, np.float64).reshape(-1, 4)
    e["c"], e["s"], e["tx"], e["ty"] = z[:, 0], z[:, 1], z[:, 2], z[:, 3]
    e["w_t"], e["w_r"] = w_t, w_r
    return e


def states_of(yaw, tx, ty):
    return np.ascontiguousarray(np.stack([np.cos(yaw), np.sin(yaw), np.asarray(tx, np.float64), np.asarray(ty, np.float64)], axis=1))


def relative(a, b):
    """the state of b in a's frame, row by row"""
    dx, dy = b[:, 2] - a[:, 2], b[:, 3] - a[:, 3]
    return np.stack([a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0], a[:, 0] * dx + a[:, 1] * dy, a[:, 0] * dy - a[:, 1] * dx], axis=1)


def compose(a, m):
    """the state that sits at m in a's frame"""
    return np.array([a[0] * m[0] - a[1] * m[1], a[1] * m[0] + a[0] * m[1], a[2] + a[0] * m[2] - a[1] * m[3], a[3] + a[1] * m[2] + a[0] * m[3]])


def noisy(rs, z, sigma_r, sigma_t):
    yaw = np.arctan2(z[:, 1], z[:, 0]) + rs.normal(0, sigma_r, len(z))
    return np.stack([np.cos(yaw), np.sin(yaw), z[:, 2] + rs.normal(0, sigma_t, len(z)), z[:, 3] + rs.normal(0, sigma_t, len(z))], axis=1)


def random_graph(seed, n_nodes, n_edges, n_fixed=1):
    """states scattered over a field, a chain through all of them and random further edges, measured with a little noise; the start is the
    truth disturbed -> (start, fixed, edges)"""
    rs = np.random.RandomState(seed)
    truth = states_of(rs.uniform(-3, 3, n_nodes), rs.uniform(-20, 20, n_nodes), rs.uniform(-20, 20, n_nodes))
    i = np.concatenate([np.arange(n_nodes - 1), rs.randint(0, n_nodes, max(n_edges - (n_nodes - 1), 0))])[:n_edges]
    j = np.concatenate([np.arange(1, n_nodes), rs.randint(0, n_nodes, max(n_edges - (n_nodes - 1), 0))])[:n_edges]
    clash = i == j
    j[clash] = (j[clash] + 1) % max(n_nodes, 2)
    if n_nodes == 1:
        i, j = i[:0], j[:0]
    z = noisy(rs, relative(truth[i], truth[j]), 0.01, 0.02)
    edges = edges_of(i, j, z, rs.uniform(20, 200, len(i)), rs.uniform(50, 500, len(i)))
    start = noisy(rs, truth, 0.05, 0.1)
    fixed = np.zeros(n_nodes, np.uint8)
    fixed[:n_fixed] = 1
    start[:n_fixed] = truth[:n_fixed]
    return start, fixed, edges


def loop_graph(seed, per_side=16, sigma_r=0.01, sigma_t=0.02, bias_r=0.004, closures=((0, -1),), outliers=(), w_t=100.0, w_r=400.0):
    """a square trajectory of 4 * per_side poses one metre apart, its odometry drifting (noise and a yaw bias per step), true closures (i, j)
    measured exactly and `outliers` (i, j, dx, dy) measured wrongly; the start is the integrated odometry, node 0 is fixed
    -> (truth, start, fixed, edges)"""
    rs = np.random.RandomState(seed)
    n = 4 * per_side
    yaw = np.repeat(np.arange(4) * (np.pi / 2), per_side)
    step = np.stack([np.cos(yaw), np.sin(yaw)], axis=1)
    pos = np.concatenate([np.zeros((1, 2)), np.cumsum(step[:-1], axis=0)])
    truth = states_of(yaw, pos[:, 0], pos[:, 1])
    a = np.arange(n - 1)
    odo = relative(truth[a], truth[a + 1])
    odo_yaw = np.arctan2(odo[:, 1], odo[:, 0]) + rs.normal(0, sigma_r, n - 1) + bias_r
    odo = np.stack([np.cos(odo_yaw), np.sin(odo_yaw), odo[:, 2] + rs.normal(0, sigma_t, n - 1), odo[:, 3] + rs.normal(0, sigma_t, n - 1)], axis=1)
    ci = np.array([c[0] % n for c in closures] + [o[0] % n for o in outliers], np.int64)
    cj = np.array([c[1] % n for c in closures] + [o[1] % n for o in outliers], np.int64)
    cz = relative(truth[ci], truth[cj])
    for k, o in enumerate(outliers):
        cz[len(closures) + k, 2:] += o[2:]
    edges = edges_of(np.concatenate([a, ci]), np.concatenate([a + 1, cj]), np.concatenate([odo, cz]), w_t, w_r)
    start = np.zeros((n, 4))
    start[0] = truth[0]
    for k in range(n - 1):
        start[k + 1] = compose(start[k], odo[k])
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return truth, start, fixed, edges


def trajectory_error(states, truth):
    """the root mean square distance of the positions from the truth, metres"""
    d = np.asarray(states)[:, 2:] - truth[:, 2:]
    return float(np.sqrt(np.mean(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])))
