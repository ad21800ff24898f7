// rr_graph.hip -- gfx950 kernels of the pose-graph optimiser (rr_graph_plan_device, rr_optimize_graph_device).  The definition is in
// include/radarays_mi355.h: f64, + - * / sqrt, every sum in a stated order, so the GPU and tests/graph_ref.py agree byte for byte.
//
// The plan, a memset of the counts, six launches and a memset of the work area:
//   k_gp_count     one thread per edge: one integer atomic per valid endpoint into the node's count
//   k_gp_chunks / k_gp_scan / k_gp_offsets   the exclusive scan of the counts (the shape of rr_surfels.hip's: per-chunk totals, one workgroup
//                  over them, ranks per chunk again): the lists' offsets, and a cursor per node
//   k_gp_fill      one thread per edge: its index behind the cursor of each endpoint, in whatever order the atomics fall
//   k_gp_sort      one thread per node: every entry's rank among its list, written to the final list -- ascending edge index whichever way
//                  the list was filled.  A list longer than kHub is ranked by its wave, a lane per entry (quadratic in the list: the plan is
//                  built once)
// The solve, per outer iteration: k_graph_linearize (one thread per edge: the edge's terms, flag and chi, the chunk's chi by the halving
// tree), k_graph_gather (one thread per node: H_nn, g_n, the LDL^T factors, r, z, x = 0), per CG step k_graph_hp (p and q = Hp by a gather
// over the plan, <p, q> partials) and k_graph_cg (x, r, z, <r, z> partials), k_graph_update, k_graph_rec.  A scalar of the CG is re-reduced
// from the chunks' partials by every workgroup that needs it, in the one stated order; whether the solve has stopped is a word per step
// (ctl[k], written by workgroup 0 of the launch before).  Values cross between workgroups at KERNEL BOUNDARIES only: no workgroup waits
// for another, no atomic takes part in the arithmetic.
// The product is matrix-free: 96 bytes of terms per edge (at 2^22 edges 3 x 3 blocks per edge and side would be close to a gigabyte).
// A node's gather is serial in its thread up to kHub entries; a longer list is taken by the whole wave, lane l its entries l, l + 64, ...
// and a halving over the lanes (list_sum), so a hub does not hold 63 lanes behind one.
// No scratch (private) memory; 2 KB of static LDS for the halving tree.
#include "../../include/radarays_mi355.h"
#include "rr_device.h"
#include "rr_launch.h"
#include "rr_pose2d.h"

namespace rr {

namespace {

constexpr int kGTB = 256;                            // threads of every workgroup here; the chunk of a reduction (node_chunk, edge_tile)
constexpr uint32_t kHub = 64;                        // a list of more entries is summed by its wave
constexpr int kGpPer = 4;                            // counts per thread of the plan's scan
constexpr int kGpChunk = kGTB * kGpPer;              // 1024: at most 1024 chunks for 2^20 nodes, one workgroup scans them
constexpr uint32_t kPlanMagic = 0x50474152u;
constexpr double kFlipDen = 1.0 / 1048576.0;         // 2^-20

static_assert(sizeof(rr_graph_edge) == 48 && sizeof(rr_graph_config) == 32 && sizeof(rr_graph_rec) == 32, "an edge: 48 bytes; a config and a record: 32");

struct alignas(16) GTerm { double ci, si, ux, uy, kk, wt, wr, etx, ety, er; uint32_t i, j; };
static_assert(sizeof(GTerm) == 96, "the terms of an edge: 96 bytes");

size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

// ---- the plan: header [4] | offsets [N + 1] | lists [2E] | work: cursor [N], tmp [2E], partials [1024] -- uint32 words, 16-byte sections ----
struct PlanLayout { size_t offsets, lists, cursor, tmp, partials, total; };
PlanLayout plan_layout(size_t N, size_t E)
{
    PlanLayout L;
    L.offsets = 16;
    L.lists = L.offsets + align16((N + 1) * 4);
    L.cursor = L.lists + align16(2 * E * 4);
    L.tmp = L.cursor + align16(N * 4);
    L.partials = L.tmp + align16(2 * E * 4);
    L.total = L.partials + 1024 * 4;
    return L;
}

__device__ inline bool edge_ends_ok(uint32_t i, uint32_t j, uint32_t N) { return i != j && i < N && j < N; }

__global__ void __launch_bounds__(kGTB) k_gp_count(const rr_graph_edge* edges, uint32_t N, uint32_t E, uint32_t* cnt)
{
    const uint32_t e = blockIdx.x * (uint32_t)kGTB + threadIdx.x;
    if (e >= E) return;
    const uint32_t i = edges[e].i, j = edges[e].j;
    if (!edge_ends_ok(i, j, N)) return;
    atomicAdd(cnt + i, 1u); atomicAdd(cnt + j, 1u);
}

__global__ void __launch_bounds__(kGTB) k_gp_chunks(const uint32_t* cnt, uint32_t N, uint32_t* partials)
{
    __shared__ int s_scan[8];
    const uint32_t n0 = blockIdx.x * (uint32_t)kGpChunk + threadIdx.x * kGpPer;
    int v = 0;
    for (int a = 0; a < kGpPer; a++) if (n0 + a < N) v += (int)cnt[n0 + a];
    int total;
    block_excl_scan(v, total, s_scan);
    if (threadIdx.x == 0) partials[blockIdx.x] = (uint32_t)total;
}

// one workgroup: the exclusive scan of at most 1024 chunk totals in place, the header, and the closing offset
__global__ void __launch_bounds__(kGTB) k_gp_scan(uint32_t* partials, uint32_t n_chunks, uint32_t N, uint32_t E, uint32_t* header, uint32_t* offsets)
{
    __shared__ int s_scan[8];
    const uint32_t b0 = threadIdx.x * kGpPer;
    int v[kGpPer], sum = 0;
    for (int a = 0; a < kGpPer; a++) { v[a] = b0 + a < n_chunks ? (int)partials[b0 + a] : 0; sum += v[a]; }
    int total;
    int ex = block_excl_scan(sum, total, s_scan);
    for (int a = 0; a < kGpPer; a++) { if (b0 + a < n_chunks) partials[b0 + a] = (uint32_t)ex; ex += v[a]; }
    if (threadIdx.x == 0) {
        header[0] = kPlanMagic; header[1] = N; header[2] = E; header[3] = 0;
        offsets[N] = (uint32_t)total;
    }
}

__global__ void __launch_bounds__(kGTB) k_gp_offsets(uint32_t* cnt_cursor, const uint32_t* partials, uint32_t N, uint32_t* offsets)
{
    __shared__ int s_scan[8];
    const uint32_t n0 = blockIdx.x * (uint32_t)kGpChunk + threadIdx.x * kGpPer;
    int v[kGpPer], sum = 0;
    for (int a = 0; a < kGpPer; a++) { v[a] = n0 + a < N ? (int)cnt_cursor[n0 + a] : 0; sum += v[a]; }
    int total;
    uint32_t at = partials[blockIdx.x] + (uint32_t)block_excl_scan(sum, total, s_scan);
    for (int a = 0; a < kGpPer; a++) {
        if (n0 + a < N) { offsets[n0 + a] = at; cnt_cursor[n0 + a] = at; }
        at += (uint32_t)v[a];
    }
}

__global__ void __launch_bounds__(kGTB) k_gp_fill(const rr_graph_edge* edges, uint32_t N, uint32_t E, uint32_t* cursor, uint32_t* tmp)
{
    const uint32_t e = blockIdx.x * (uint32_t)kGTB + threadIdx.x;
    if (e >= E) return;
    const uint32_t i = edges[e].i, j = edges[e].j;
    if (!edge_ends_ok(i, j, N)) return;
    const uint32_t a = atomicAdd(cursor + i, 1u), b = atomicAdd(cursor + j, 1u);
    if (a < 2 * E) tmp[a] = e;                                    // (the counts of the same edges: always within the list)
    if (b < 2 * E) tmp[b] = e;
}

// entries start, start + stride, .. of a list to their ranks (an edge index appears once in a node's list: i != j)
__device__ inline void rank_entries(const uint32_t* src, uint32_t* dst, uint32_t len, uint32_t start, uint32_t stride)
{
    for (uint32_t a = start; a < len; a += stride) {
        const uint32_t e = src[a];
        uint32_t rank = 0;
        for (uint32_t b = 0; b < len; b++) rank += src[b] < e ? 1u : 0u;
        dst[rank] = e;
    }
}

__global__ void __launch_bounds__(kGTB) k_gp_sort(const uint32_t* offsets, const uint32_t* tmp, uint32_t* lists, uint32_t N)
{
    const uint32_t n = blockIdx.x * (uint32_t)kGTB + threadIdx.x;
    const bool valid = n < N;
    const uint32_t beg = valid ? offsets[n] : 0u, len = valid ? offsets[n + 1] - beg : 0u;
    if (len <= kHub) rank_entries(tmp + beg, lists + beg, len, 0, 1);
    const int lane = threadIdx.x & 63;
    unsigned long long hubs = __ballot(len > kHub);
    while (hubs) {
        const int b = __ffsll(hubs) - 1;
        hubs &= hubs - 1;
        const uint32_t hbeg = __shfl(beg, b, 64), hlen = __shfl(len, b, 64);
        rank_entries(tmp + hbeg, lists + hbeg, hlen, (uint32_t)lane, 64);
    }
}

// ---- the solve -------------------------------------------------------------------------------------------------------------------------
struct GraphArgs {
    uint32_t N, E, NC, EC;                           // nodes, edges, chunks of kGTB of each
    int cg_iterations;
    double lambda, k2;                               // k2 = robust_k * robust_k, 0: no kernel
    double* states; const uint8_t* fixed; const rr_graph_edge* edges;
    const uint32_t *plan_header, *offsets, *lists;
    uint8_t* edge_flags;                             // the caller's plane, or null
    // the scratch
    GTerm* terms; uint8_t* eflag; double* chi_part; uint32_t* cnt_part;      // [E] [E] [EC] [EC][3]
    double *x, *r, *z, *p[2], *q; Ldl3* fac; uint8_t* nstate;               // [N][3] each, [N], [N]: 0 active, 1 fixed, 2 dead
    double *rz_part[2], *pq_part; uint32_t* dead_part;                      // [NC] each
    int* ctl; double* rzs;                                                   // [cg_iterations + 1], [cg_iterations + 1]
};

struct SolveLayout { size_t terms, eflag, chi_part, cnt_part, vec[6], fac, nstate, rz_part[2], pq_part, dead_part, ctl, rzs, total; };
SolveLayout solve_layout(size_t N, size_t E, size_t cg)
{
    const size_t NC = (N + kGTB - 1) / kGTB, EC = (E + kGTB - 1) / kGTB;
    SolveLayout L;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += align16(bytes); return o; };
    L.terms = take(E * sizeof(GTerm)); L.eflag = take(E); L.chi_part = take(EC * 8); L.cnt_part = take(EC * 12);
    for (int k = 0; k < 6; k++) L.vec[k] = take(N * 24);
    L.fac = take(N * sizeof(Ldl3)); L.nstate = take(N);
    L.rz_part[0] = take(NC * 8); L.rz_part[1] = take(NC * 8); L.pq_part = take(NC * 8); L.dead_part = take(NC * 4);
    L.ctl = take((cg + 1) * 4); L.rzs = take((cg + 1) * 8);
    L.total = at;
    return L;
}

// the halving tree of the header over the workgroup's 256 values: v[t] = v[t] + v[t + h], h = 128 .. 1; v[0] is returned to every thread.
// Every thread of the workgroup calls it
__device__ inline double block_tree_sum(double x, double* lds /*[kGTB]*/)
{
    const int t = threadIdx.x;
    lds[t] = x;
    __syncthreads();
    if (t < 128) lds[t] = lds[t] + lds[t + 128];
    __syncthreads();
    double v = 0.0;
    if (t < 64) {
        v = lds[t] + lds[t + 64];
        for (int h = 32; h > 0; h >>= 1) v = v + __shfl_down(v, h, 64);
    }
    __syncthreads();
    if (t == 0) lds[0] = v;
    __syncthreads();
    v = lds[0];
    __syncthreads();
    return v;
}

// the partials P[0 .. m) combined as the header says: s[t] = P[t] + P[t + 256] + .. one after the other from 0.0, then the halving tree
__device__ inline double combine(const double* part, uint32_t m, double* lds)
{
    double s = 0.0;
    for (uint32_t a = threadIdx.x; a < m; a += kGTB) s = s + part[a];
    return block_tree_sum(s, lds);
}

__device__ inline bool finite_d(double v) { return fabs(v) < (double)INFINITY; }      // false for NaN and infinities
__device__ inline bool finite_f(float v) { return fabsf(v) < INFINITY; }

__global__ void __launch_bounds__(kGTB) k_graph_linearize(GraphArgs A)
{
    __shared__ double s_tree[kGTB];
    __shared__ uint32_t s_cnt[4][3];
    const uint32_t e = blockIdx.x * (uint32_t)kGTB + threadIdx.x;
    double chi = 0.0;
    uint32_t flag = 0, valid = e < A.E ? 1u : 0u;
    if (valid) {
        const rr_graph_edge ed = A.edges[e];
        GTerm T = {};
        T.i = ed.i; T.j = ed.j;
        if (!edge_ends_ok(ed.i, ed.j, A.N) || !(finite_d(ed.c) && finite_d(ed.s) && finite_d(ed.tx) && finite_d(ed.ty)) ||
            !(finite_f(ed.w_t) && finite_f(ed.w_r) && ed.w_t >= 0.0f && ed.w_r >= 0.0f)) {
            flag = RR_GRAPH_EDGE_BAD;
        } else {
            const double* si_ = A.states + 4 * (size_t)ed.i; const double* sj_ = A.states + 4 * (size_t)ed.j;
            const double ci = si_[0], si = si_[1], cj = sj_[0], sj = sj_[1];
            const double dx = sj_[2] - si_[2], dy = sj_[3] - si_[3];
            const double ux = ci * dx + si * dy, uy = ci * dy - si * dx;
            const double etx = ux - ed.tx, ety = uy - ed.ty;
            const double a = ci * cj + si * sj, b = ci * sj - si * cj;
            const double rc = ed.c * a + ed.s * b, rs = ed.c * b - ed.s * a;
            const double den = 1.0 + rc;
            if (!(den >= kFlipDen)) {
                flag = RR_GRAPH_EDGE_FLIPPED;
            } else {
                const double er = (2.0 * rs) / den;
                double wt = (double)ed.w_t, wr = (double)ed.w_r;
                const double ch = wt * (etx * etx + ety * ety) + wr * (er * er);
                if (!finite_d(ch)) {
                    flag = RR_GRAPH_EDGE_BAD;
                } else {
                    chi = ch;
                    if (A.k2 > 0.0) { const double sc = 1.0 / (1.0 + ch / A.k2); wt = wt * sc; wr = wr * sc; }
                    T.ci = ci; T.si = si; T.ux = ux; T.uy = uy; T.kk = 1.0 + (er * er) / 4.0; T.wt = wt; T.wr = wr;
                    T.etx = etx; T.ety = ety; T.er = er;
                }
            }
        }
        A.terms[e] = T;
        A.eflag[e] = (uint8_t)flag;
        if (A.edge_flags) A.edge_flags[e] = (uint8_t)flag;
    }
    const double part = block_tree_sum(chi, s_tree);
    const uint32_t used = wave_sum(valid && flag == 0 ? 1u : 0u), flipped = wave_sum(flag == RR_GRAPH_EDGE_FLIPPED ? 1u : 0u),
                   bad = wave_sum(flag == RR_GRAPH_EDGE_BAD ? 1u : 0u);
    if ((threadIdx.x & 63) == 0) { uint32_t* c = s_cnt[threadIdx.x >> 6]; c[0] = used; c[1] = flipped; c[2] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) A.chi_part[blockIdx.x] = part;
    if (threadIdx.x < 3) A.cnt_part[3 * (size_t)blockIdx.x + threadIdx.x] = s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
}

// a node's list in the plan, cut to the plan's own bounds (a plan of another graph gives empty lists, never an address outside)
__device__ inline void node_list(const GraphArgs& A, uint32_t n, bool valid, uint32_t& beg, uint32_t& len)
{
    beg = 0; len = 0;
    if (!valid || A.plan_header[0] != kPlanMagic || A.plan_header[1] != A.N || A.plan_header[2] != A.E) return;
    const uint32_t cap = 2 * A.E, b = min(A.offsets[n], cap), e = min(A.offsets[n + 1], cap);
    if (e > b) { beg = b; len = e - b; }
}

// the LIST SUM of the header: out[0 .. K) of node n over its list; f(e, n, term) gives edge e's term as node n, false for a flagged edge.
// Every lane of the wave calls it (valid: this lane has a node to sum)
template <int K, class F> __device__ inline void list_sum(const GraphArgs& A, uint32_t n, bool valid, uint32_t beg, uint32_t len, F f, double* out)
{
    for (int k = 0; k < K; k++) out[k] = 0.0;
    const bool is_long = valid && len > kHub;
    if (valid && !is_long)
        for (uint32_t a = 0; a < len; a++) {
            const uint32_t e = A.lists[beg + a];
            double c[K];
            if (e < A.E && f(e, n, c)) for (int k = 0; k < K; k++) out[k] = out[k] + c[k];
        }
    const int lane = threadIdx.x & 63;
    unsigned long long hubs = __ballot(is_long);
    while (hubs) {
        const int b = __ffsll(hubs) - 1;
        hubs &= hubs - 1;
        const uint32_t hn = __shfl(n, b, 64), hbeg = __shfl(beg, b, 64), hlen = __shfl(len, b, 64);
        double acc[K];
        for (int k = 0; k < K; k++) acc[k] = 0.0;
        for (uint32_t a = (uint32_t)lane; a < hlen; a += 64) {
            const uint32_t e = A.lists[hbeg + a];
            double c[K];
            if (e < A.E && f(e, hn, c)) for (int k = 0; k < K; k++) acc[k] = acc[k] + c[k];
        }
        for (int k = 0; k < K; k++) {
            for (int h = 32; h > 0; h >>= 1) acc[k] = acc[k] + __shfl_down(acc[k], h, 64);
            const double total = __shfl(acc[k], 0, 64);
            if (lane == b) out[k] = total;
        }
    }
}

__device__ inline double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__global__ void __launch_bounds__(kGTB) k_graph_gather(GraphArgs A)
{
    __shared__ double s_tree[kGTB];
    __shared__ uint32_t s_dead[4];
    const uint32_t n = blockIdx.x * (uint32_t)kGTB + threadIdx.x;
    const bool valid = n < A.N, free_ = valid && A.fixed[n] == 0;
    uint32_t beg, len;
    node_list(A, n, free_, beg, len);
    double S[7];                                                     // H00 H01 H02 H11 g0 g1 g2
    list_sum<7>(A, n, free_, beg, len, [&](uint32_t e, uint32_t node, double* c) {
        if (A.eflag[e]) return false;
        const GTerm T = A.terms[e];
        const double nn = T.ci * T.ci + T.si * T.si;
        if (T.i == node) {
            c[0] = T.wt * (T.uy * T.uy + T.ux * T.ux) + T.wr * (T.kk * T.kk);
            c[1] = -(T.wt * (T.uy * T.ci + T.ux * T.si));
            c[2] = T.wt * (T.ux * T.ci - T.uy * T.si);
            c[3] = T.wt * nn;
            c[4] = T.wt * (T.uy * T.etx - T.ux * T.ety) - T.wr * (T.kk * T.er);
            c[5] = T.wt * (T.si * T.ety - T.ci * T.etx);
            c[6] = -(T.wt * (T.si * T.etx + T.ci * T.ety));
        } else {
            c[0] = T.wr * (T.kk * T.kk); c[1] = 0.0; c[2] = 0.0;
            c[3] = T.wt * nn;
            c[4] = T.wr * (T.kk * T.er);
            c[5] = T.wt * (T.ci * T.etx - T.si * T.ety);
            c[6] = T.wt * (T.si * T.etx + T.ci * T.ety);
        }
        return true;
    }, S);
    double rz = 0.0;
    uint32_t dead = 0;
    if (valid) {
        double r[3] = { 0.0, 0.0, 0.0 }, z[3] = { 0.0, 0.0, 0.0 };
        Ldl3 f = {};
        uint8_t state = 1;
        if (free_) {
            const double d = S[3] + A.lambda;
            if (ldl3_factor(S[0] + A.lambda, S[1], S[2], d, d, f)) {
                state = 0;
                r[0] = -S[4]; r[1] = -S[5]; r[2] = -S[6];
                ldl3_solve(f, r, z);
                rz = dot3(r, z);
            } else {
                state = 2; dead = 1;
            }
        }
        A.nstate[n] = state;
        A.fac[n] = f;
        for (int k = 0; k < 3; k++) { A.x[3 * (size_t)n + k] = 0.0; A.r[3 * (size_t)n + k] = r[k]; A.z[3 * (size_t)n + k] = z[k]; }
    }
    const double part = block_tree_sum(rz, s_tree);
    dead = wave_sum(dead);
    if ((threadIdx.x & 63) == 0) s_dead[threadIdx.x >> 6] = dead;
    __syncthreads();
    if (threadIdx.x == 0) {
        A.rz_part[0][blockIdx.x] = part;
        A.dead_part[blockIdx.x] = s_dead[0] + s_dead[1] + s_dead[2] + s_dead[3];
        if (blockIdx.x == 0) A.ctl[0] = -1;
    }
}

// CG step k, first half: p (own, written to p[k & 1]; a neighbour's recomputed from z and the p before), q = Hp + lambda p, <p, q> partials
__global__ void __launch_bounds__(kGTB) k_graph_hp(GraphArgs A, int k)
{
    __shared__ double s_tree[kGTB];
    if (A.ctl[k] >= 0) return;                                        // (the whole grid: the solve has stopped)
    const double rz = combine(A.rz_part[k & 1], A.NC, s_tree);
    const double beta = k > 0 ? rz / A.rzs[k - 1] : 0.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) A.rzs[k] = rz;
    const double* pold = A.p[(k + 1) & 1];
    auto p_of = [&](uint32_t m, double* out) {
        for (int c = 0; c < 3; c++) {
            const double z = A.z[3 * (size_t)m + c];
            out[c] = k > 0 ? z + beta * pold[3 * (size_t)m + c] : z;
        }
    };
    const uint32_t n = blockIdx.x * (uint32_t)kGTB + threadIdx.x;
    const bool valid = n < A.N, active = valid && A.nstate[n] == 0;
    double pn[3] = { 0.0, 0.0, 0.0 }, q[3];
    if (valid) p_of(n, pn);
    uint32_t beg, len;
    node_list(A, n, active, beg, len);
    list_sum<3>(A, n, active, beg, len, [&](uint32_t e, uint32_t node, double* c) {
        if (A.eflag[e]) return false;
        const GTerm T = A.terms[e];
        double pi[3], pj[3];
        p_of(T.i, pi); p_of(T.j, pj);
        const double v0 = ((T.uy * pi[0] - T.ci * pi[1]) - T.si * pi[2]) + (T.ci * pj[1] + T.si * pj[2]);
        const double v1 = ((T.si * pi[1] - T.ux * pi[0]) - T.ci * pi[2]) + (T.ci * pj[2] - T.si * pj[1]);
        const double v2 = T.kk * (pj[0] - pi[0]);
        const double y0 = T.wt * v0, y1 = T.wt * v1, y2 = T.wr * v2;
        if (T.i == node) {
            c[0] = (T.uy * y0 - T.ux * y1) - T.kk * y2;
            c[1] = T.si * y1 - T.ci * y0;
            c[2] = -(T.si * y0 + T.ci * y1);
        } else {
            c[0] = T.kk * y2;
            c[1] = T.ci * y0 - T.si * y1;
            c[2] = T.si * y0 + T.ci * y1;
        }
        return true;
    }, q);
    double pq = 0.0;
    if (valid) {
        if (active) { for (int c = 0; c < 3; c++) q[c] = q[c] + A.lambda * pn[c]; pq = dot3(pn, q); }
        else q[0] = q[1] = q[2] = 0.0;
        double* pnew = A.p[k & 1];
        for (int c = 0; c < 3; c++) { pnew[3 * (size_t)n + c] = pn[c]; A.q[3 * (size_t)n + c] = q[c]; }
    }
    const double part = block_tree_sum(pq, s_tree);
    if (threadIdx.x == 0) A.pq_part[blockIdx.x] = part;
}

// CG step k, second half: alpha, x, r, z = M^-1 r, <r, z> partials; workgroup 0 hands the stop word on
__global__ void __launch_bounds__(kGTB) k_graph_cg(GraphArgs A, int k)
{
    __shared__ double s_tree[kGTB];
    const int stopped = A.ctl[k];
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (stopped >= 0) { if (first) A.ctl[k + 1] = stopped; return; }
    const double pAp = combine(A.pq_part, A.NC, s_tree), rz = A.rzs[k];
    if (!(pAp > 0.0 && pAp < (double)INFINITY && rz > 0.0 && rz < (double)INFINITY)) { if (first) A.ctl[k + 1] = k; return; }
    const double alpha = rz / pAp;
    const uint32_t n = blockIdx.x * (uint32_t)kGTB + threadIdx.x;
    double rz1 = 0.0;
    if (n < A.N && A.nstate[n] == 0) {
        const double* p = A.p[k & 1] + 3 * (size_t)n;
        double r[3], z[3];
        for (int c = 0; c < 3; c++) {
            A.x[3 * (size_t)n + c] = A.x[3 * (size_t)n + c] + alpha * p[c];
            r[c] = A.r[3 * (size_t)n + c] - alpha * A.q[3 * (size_t)n + c];
            A.r[3 * (size_t)n + c] = r[c];
        }
        ldl3_solve(A.fac[n], r, z);
        for (int c = 0; c < 3; c++) A.z[3 * (size_t)n + c] = z[c];
        rz1 = dot3(r, z);
    }
    const double part = block_tree_sum(rz1, s_tree);
    if (threadIdx.x == 0) A.rz_part[(k + 1) & 1][blockIdx.x] = part;
    if (first) A.ctl[k + 1] = -1;
}

__global__ void __launch_bounds__(kGTB) k_graph_update(GraphArgs A)
{
    const uint32_t n = blockIdx.x * (uint32_t)kGTB + threadIdx.x;
    if (n >= A.N || A.nstate[n] != 0) return;
    const double dth = A.x[3 * (size_t)n], dx = A.x[3 * (size_t)n + 1], dy = A.x[3 * (size_t)n + 2];
    if (dth == 0.0 && dx == 0.0 && dy == 0.0) return;
    double* st = A.states + 4 * (size_t)n;
    const double c = st[0], s = st[1];
    const double u = dth / 2.0;
    const double dc = (1.0 - u * u) / (1.0 + u * u), ds = (2.0 * u) / (1.0 + u * u);
    const double c1 = c * dc - s * ds, s1 = s * dc + c * ds;
    const double nrm = sqrt(c1 * c1 + s1 * s1);
    st[0] = c1 / nrm; st[1] = s1 / nrm; st[2] = st[2] + dx; st[3] = st[3] + dy;
}

// one workgroup: the record of an outer iteration (last: of the final states)
__global__ void __launch_bounds__(kGTB) k_graph_rec(GraphArgs A, rr_graph_rec* rec, int last)
{
    __shared__ double s_tree[kGTB];
    __shared__ uint32_t s_cnt[4][4];
    const double chi2 = combine(A.chi_part, A.EC, s_tree);
    uint32_t cnt[4] = { 0, 0, 0, 0 };
    for (uint32_t a = threadIdx.x; a < A.EC; a += kGTB) for (int k = 0; k < 3; k++) cnt[k] += A.cnt_part[3 * (size_t)a + k];
    if (!last) for (uint32_t a = threadIdx.x; a < A.NC; a += kGTB) cnt[3] += A.dead_part[a];
    for (int k = 0; k < 4; k++) cnt[k] = wave_sum(cnt[k]);
    if ((threadIdx.x & 63) == 0) for (int k = 0; k < 4; k++) s_cnt[threadIdx.x >> 6][k] = cnt[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        rr_graph_rec r;
        r.chi2 = chi2;
        r.n_used = s_cnt[0][0] + s_cnt[1][0] + s_cnt[2][0] + s_cnt[3][0];
        r.n_flipped = s_cnt[0][1] + s_cnt[1][1] + s_cnt[2][1] + s_cnt[3][1];
        r.n_bad = s_cnt[0][2] + s_cnt[1][2] + s_cnt[2][2] + s_cnt[3][2];
        r.n_dead = s_cnt[0][3] + s_cnt[1][3] + s_cnt[2][3] + s_cnt[3][3];
        r.cg_stop = last ? -1 : A.ctl[A.cg_iterations];
        r.reserved_ = 0;
        *rec = r;
    }
}

}  // namespace

void graph_tile_sizes(int* node_chunk, int* edge_tile)
{
    if (node_chunk) *node_chunk = kGTB;
    if (edge_tile) *edge_tile = kGTB;
}

size_t graph_plan_bytes(size_t n_nodes, size_t n_edges) { return plan_layout(n_nodes, n_edges).total; }
size_t graph_scratch_bytes(size_t n_nodes, size_t n_edges, size_t cg_iterations) { return solve_layout(n_nodes, n_edges, cg_iterations).total; }

hipError_t launch_graph_plan(const rr_graph_edge* edges, int n_nodes, int n_edges, void* plan, hipStream_t s)
{
    const uint32_t N = (uint32_t)n_nodes, E = (uint32_t)n_edges;
    const PlanLayout L = plan_layout(N, E);
    uint8_t* base = static_cast<uint8_t*>(plan);
    uint32_t *header = reinterpret_cast<uint32_t*>(base), *offsets = reinterpret_cast<uint32_t*>(base + L.offsets),
             *lists = reinterpret_cast<uint32_t*>(base + L.lists), *cursor = reinterpret_cast<uint32_t*>(base + L.cursor),
             *tmp = reinterpret_cast<uint32_t*>(base + L.tmp), *partials = reinterpret_cast<uint32_t*>(base + L.partials);
    // every byte of the plan is written: the sections' padding with the rest
    hipError_t err = hipMemsetAsync(plan, 0, L.total, s);
    if (err != hipSuccess) return err;
    const unsigned eg = (E + kGTB - 1) / kGTB, ng = (N + kGTB - 1) / kGTB, chunks = (N + kGpChunk - 1) / kGpChunk;
    if (eg) hipLaunchKernelGGL(k_gp_count, dim3(eg), dim3(kGTB), 0, s, edges, N, E, cursor);
    hipLaunchKernelGGL(k_gp_chunks, dim3(chunks), dim3(kGTB), 0, s, (const uint32_t*)cursor, N, partials);
    hipLaunchKernelGGL(k_gp_scan, dim3(1), dim3(kGTB), 0, s, partials, chunks, N, E, header, offsets);
    hipLaunchKernelGGL(k_gp_offsets, dim3(chunks), dim3(kGTB), 0, s, cursor, (const uint32_t*)partials, N, offsets);
    if (eg) {
        hipLaunchKernelGGL(k_gp_fill, dim3(eg), dim3(kGTB), 0, s, edges, N, E, cursor, tmp);
        hipLaunchKernelGGL(k_gp_sort, dim3(ng), dim3(kGTB), 0, s, (const uint32_t*)offsets, (const uint32_t*)tmp, lists, N);
    }
    // the work area held whatever order the atomics fell in: cleared, so that the plan's bytes are a function of the endpoints
    return hipMemsetAsync(base + L.cursor, 0, L.total - L.cursor, s);
}

void launch_optimize_graph(double* states, const uint8_t* fixed, const rr_graph_edge* edges, int n_nodes, int n_edges, const void* plan,
                           const rr_graph_config& cfg, rr_graph_rec* recs, uint8_t* edge_flags, void* scratch, hipStream_t s)
{
    GraphArgs A;
    A.N = (uint32_t)n_nodes; A.E = (uint32_t)n_edges;
    A.NC = (A.N + kGTB - 1) / kGTB; A.EC = (A.E + kGTB - 1) / kGTB;
    A.cg_iterations = cfg.cg_iterations; A.lambda = cfg.lambda; A.k2 = cfg.robust_k * cfg.robust_k;
    A.states = states; A.fixed = fixed; A.edges = edges; A.edge_flags = edge_flags;
    const PlanLayout P = plan_layout(A.N, A.E);
    const uint8_t* pb = static_cast<const uint8_t*>(plan);
    A.plan_header = reinterpret_cast<const uint32_t*>(pb);
    A.offsets = reinterpret_cast<const uint32_t*>(pb + P.offsets);
    A.lists = reinterpret_cast<const uint32_t*>(pb + P.lists);
    const SolveLayout L = solve_layout(A.N, A.E, (size_t)cfg.cg_iterations);
    uint8_t* sb = static_cast<uint8_t*>(scratch);
    A.terms = reinterpret_cast<GTerm*>(sb + L.terms); A.eflag = sb + L.eflag;
    A.chi_part = reinterpret_cast<double*>(sb + L.chi_part); A.cnt_part = reinterpret_cast<uint32_t*>(sb + L.cnt_part);
    double* vec[6];
    for (int k = 0; k < 6; k++) vec[k] = reinterpret_cast<double*>(sb + L.vec[k]);
    A.x = vec[0]; A.r = vec[1]; A.z = vec[2]; A.p[0] = vec[3]; A.p[1] = vec[4]; A.q = vec[5];
    A.fac = reinterpret_cast<Ldl3*>(sb + L.fac); A.nstate = sb + L.nstate;
    A.rz_part[0] = reinterpret_cast<double*>(sb + L.rz_part[0]); A.rz_part[1] = reinterpret_cast<double*>(sb + L.rz_part[1]);
    A.pq_part = reinterpret_cast<double*>(sb + L.pq_part); A.dead_part = reinterpret_cast<uint32_t*>(sb + L.dead_part);
    A.ctl = reinterpret_cast<int*>(sb + L.ctl); A.rzs = reinterpret_cast<double*>(sb + L.rzs);

    const dim3 tb(kGTB), eg(A.EC), ng(A.NC);
    for (int it = 0; it <= cfg.iterations; it++) {
        const int last = it == cfg.iterations;
        if (A.EC) hipLaunchKernelGGL(k_graph_linearize, eg, tb, 0, s, A);
        if (!last) {
            hipLaunchKernelGGL(k_graph_gather, ng, tb, 0, s, A);
            for (int k = 0; k < cfg.cg_iterations; k++) {
                hipLaunchKernelGGL(k_graph_hp, ng, tb, 0, s, A, k);
                hipLaunchKernelGGL(k_graph_cg, ng, tb, 0, s, A, k);
            }
            hipLaunchKernelGGL(k_graph_update, ng, tb, 0, s, A);
        }
        hipLaunchKernelGGL(k_graph_rec, dim3(1), tb, 0, s, A, recs + it, last);
    }
}

}  // namespace rr
