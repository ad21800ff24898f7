// rr_filter.hip -- gfx950 kernels of the particle filter step (rr_filter_resample_device, rr_filter_move_device; the definition is in
// include/radarays_mi355.h): the records of rr_score_poses turned into integer weights, systematically resampled, and the survivors moved
// by odometry plus diffusion.  Nothing leaves HBM; every result is an integer or a correctly rounded f32 expression.
//
// The resampler is a reduce-then-scan in SEPARATE launches: no kernel waits on another workgroup, there is no look-back and no flag.
//   k_flt_init        one thread: the summary's starting values (the reductions below are integer atomics into it)
//   k_flt_min         dmin = min sum_d2: eight records per thread, a wave minimum by shuffles, one 64-bit atomicMin per wave
//   k_flt_tile        a workgroup per scan tile (kFltTile records, eight consecutive ones per thread): the weights w_i from the table, the
//                     tile's sum written to cum[last index of the tile] -- the caller's cum is the only room the scan has --, sum w^2 by one
//                     64-bit atomicAdd per wave, `best` by one 32-bit atomicMin per wave that holds a minimum
//   k_flt_tiles       ONE workgroup: the inclusive scan of the at most kFltTile tile sums, in place.  What it leaves at the last index of
//                     tile b is cum at that index, final; cum[n - 1] is W
//   k_flt_cum         a workgroup per tile again: the weights recomputed (a table look-up is cheaper than 4 bytes of traffic each way), the scan
//                     inside the tile, plus cum[last index of tile b - 1].  The tile's own last index is not written: it is final already and the
//                     next tile is reading it
//   k_flt_draw        one thread per draw: t_j, then a plain binary search of cum in global memory (about log2 n dependent loads, the upper
//                     levels shared by the whole wave and served by L2); n_unique from the neighbour's ancestor (LDS), one atomicAdd per wave
//   k_flt_move        one thread per draw: a 16-byte load through the ancestor, the hash, the move, a 16-byte store
//
// Every scalar travels as a kernel argument.  No scratch memory in any kernel of the file.
#include "../../include/radarays_mi355.h"
#include "rr_device.h"
#include "rr_launch.h"
#include "rr_pose2d.h"

namespace rr {

namespace {

constexpr int kFltTB = 256;                      // threads of every workgroup here: four waves
constexpr int kFltPer = 8;                       // consecutive records a thread owns in the scan kernels
constexpr int kFltTile = kFltTB * kFltPer;       // 2048: the scan tile; 2^22 records are 2048 tiles, which ONE workgroup scans the same way
constexpr int kFltDraws = kFltTB;                // draws per workgroup of k_flt_draw

static_assert(sizeof(rr_field_rec) == 16 && sizeof(rr_filter_config) == 32 && sizeof(rr_filter_summary) == 32, "the records of the header");
static_assert((1 << 22) / kFltTile <= kFltTile, "one workgroup scans every tile sum");

using u64 = unsigned long long;

// the inclusive scan of one value per thread over the workgroup; total: the sum over all of it.  lds [4] may be reused after the call
__device__ inline u64 block_incl_scan(u64 v, u64* lds, u64& total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    u64 x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const u64 y = __shfl_up(x, off); if (lane >= off) x += y; }
    if (lane == 63) lds[w] = x;
    __syncthreads();
    u64 base = 0; total = 0;
#pragma unroll
    for (int k = 0; k < kFltTB / 64; k++) { const u64 t = lds[k]; if (k < w) base += t; total += t; }
    __syncthreads();
    return x + base;
}

// w_i of the header: idx = min(n_table - 1, (d2 - dmin) / quantum).  quantum * n_table < 2^43; the quotient is taken in 32 bits where it fits
__device__ inline uint32_t weight_of(u64 d2, u64 dmin, uint32_t quantum, uint32_t n_table, const uint16_t* __restrict__ table)
{
    const u64 diff = d2 - dmin;
    uint32_t idx = n_table - 1;
    if (diff < (u64)quantum * n_table) idx = (diff >> 32) == 0 ? (uint32_t)diff / quantum : (uint32_t)(diff / quantum);
    return table[idx];
}

// the last index of tile b among n records
__device__ inline uint32_t tile_last(uint32_t b, uint32_t n) { return min(b * (uint32_t)kFltTile + (uint32_t)(kFltTile - 1), n - 1); }

__global__ void k_flt_init(rr_filter_summary* sum)
{
    sum->min_sum_d2 = ~0ull; sum->total_weight = 0; sum->sum_w2 = 0; sum->best = ~0u; sum->n_unique = 1;
}

__global__ void __launch_bounds__(kFltTB) k_flt_min(const rr_field_rec* __restrict__ recs, uint32_t n, rr_filter_summary* sum)
{
    const uint32_t i0 = ((uint32_t)blockIdx.x * kFltTB + threadIdx.x) * kFltPer;
    u64 m = ~0ull;
#pragma unroll
    for (int e = 0; e < kFltPer; e++)
        if (i0 + e < n) m = min(m, (u64)recs[i0 + e].sum_d2);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = min(m, (u64)__shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0 && i0 < n) atomicMin(reinterpret_cast<u64*>(&sum->min_sum_d2), m);
}

__global__ void __launch_bounds__(kFltTB) k_flt_tile(const rr_field_rec* __restrict__ recs, uint32_t n, const uint16_t* __restrict__ table,
                                                     uint32_t quantum, uint32_t n_table, rr_filter_summary* sum, uint64_t* __restrict__ cum)
{
    __shared__ u64 lds[kFltTB / 64];
    const u64 dmin = sum->min_sum_d2;                             // k_flt_min's, a launch ago
    const uint32_t i0 = ((uint32_t)blockIdx.x * kFltTB + threadIdx.x) * kFltPer;
    u64 s = 0, s2 = 0;
    uint32_t best = ~0u;
#pragma unroll
    for (int e = kFltPer - 1; e >= 0; e--) {
        if (i0 + e >= n) continue;
        const u64 d2 = recs[i0 + e].sum_d2;
        const u64 w = weight_of(d2, dmin, quantum, n_table, table);
        s += w; s2 += w * w;
        if (d2 == dmin) best = i0 + e;                           // e runs downwards: the lowest index stays
    }
    u64 total;
    block_incl_scan(s, lds, total);
    if (threadIdx.x == 0) cum[tile_last(blockIdx.x, n)] = total;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) best = min(best, (uint32_t)__shfl_xor(best, off));
    s2 = wave_sum(s2);
    if ((threadIdx.x & 63) == 0) {
        if (s2) atomicAdd(reinterpret_cast<u64*>(&sum->sum_w2), s2);
        if (best != ~0u) atomicMin(&sum->best, best);
    }
}

__global__ void __launch_bounds__(kFltTB) k_flt_tiles(uint32_t n, rr_filter_summary* sum, uint64_t* cum)
{
    __shared__ u64 lds[kFltTB / 64];
    const uint32_t n_tiles = (n + kFltTile - 1) / kFltTile;      // at most kFltTile
    const uint32_t b0 = threadIdx.x * kFltPer;
    u64 v[kFltPer], s = 0;
#pragma unroll
    for (int e = 0; e < kFltPer; e++) { v[e] = b0 + e < n_tiles ? cum[tile_last(b0 + e, n)] : 0; s += v[e]; v[e] = s; }
    u64 total;
    const u64 base = block_incl_scan(s, lds, total) - s;
#pragma unroll
    for (int e = 0; e < kFltPer; e++)
        if (b0 + e < n_tiles) cum[tile_last(b0 + e, n)] = base + v[e];
    if (threadIdx.x == 0) sum->total_weight = total;
}

__global__ void __launch_bounds__(kFltTB) k_flt_cum(const rr_field_rec* __restrict__ recs, uint32_t n, const uint16_t* __restrict__ table,
                                                    uint32_t quantum, uint32_t n_table, const rr_filter_summary* sum, uint64_t* cum)
{
    __shared__ u64 lds[kFltTB / 64];
    const u64 dmin = sum->min_sum_d2;
    const uint32_t b = blockIdx.x, i0 = (b * kFltTB + threadIdx.x) * kFltPer, last = tile_last(b, n);
    u64 v[kFltPer], s = 0;
#pragma unroll
    for (int e = 0; e < kFltPer; e++) {
        if (i0 + e < n) s += weight_of(recs[i0 + e].sum_d2, dmin, quantum, n_table, table);
        v[e] = s;
    }
    u64 total;
    const u64 base = block_incl_scan(s, lds, total) - s + (b ? cum[b * (uint32_t)kFltTile - 1] : 0);   // the tile before: final, and nobody writes it here
#pragma unroll
    for (int e = 0; e < kFltPer; e++)
        if (i0 + e < n && i0 + e != last) cum[i0 + e] = base + v[e];
}

// numpy's searchsorted(cum, t, side='right'), clamped to n - 1
__device__ inline uint32_t draw_search(const uint64_t* __restrict__ cum, uint32_t n, u64 t)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((u64)cum[mid] <= t) lo = mid + 1; else hi = mid;
    }
    return min(lo, n - 1);
}

__global__ void __launch_bounds__(kFltDraws) k_flt_draw(const uint64_t* __restrict__ cum, uint32_t n, uint32_t n_out, uint32_t phase,
                                                        rr_filter_summary* sum, uint32_t* __restrict__ ancestors)
{
    __shared__ uint32_t anc[kFltDraws];
    const u64 W = sum->total_weight, r = ((u64)phase * W) >> 24;
    const uint32_t j = (uint32_t)blockIdx.x * kFltDraws + threadIdx.x;
    uint32_t a = 0;
    if (j < n_out) {
        a = draw_search(cum, n, ((u64)j * W + r) / n_out);
        ancestors[j] = a;
    }
    anc[threadIdx.x] = a;
    __syncthreads();
    bool fresh = false;
    if (j < n_out && j > 0) {
        const uint32_t prev = threadIdx.x ? anc[threadIdx.x - 1] : draw_search(cum, n, ((u64)(j - 1) * W + r) / n_out);
        fresh = prev != a;
    }
    const u64 mask = __ballot(fresh);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(&sum->n_unique, (uint32_t)__popcll(mask));
}

__device__ inline uint32_t mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

// v_k of the header: four 16-bit uniforms of two hashes, centred
__device__ inline float variate(uint32_t key, uint32_t j, uint32_t k)
{
    const uint32_t h = mix32(key ^ (8u * j + 2u * k)), g = mix32(key ^ (8u * j + 2u * k + 1u));
    return (float)((int)((h & 0xffffu) + (h >> 16) + (g & 0xffffu) + (g >> 16)) - 131070);
}

// un-fused f32 in the header's order; `/` and sqrtf are the correctly rounded ones (no fast-math in FLAGS)
__global__ void __launch_bounds__(kFltTB) k_flt_move(const float4* __restrict__ in, uint32_t n, const uint32_t* __restrict__ ancestors, uint32_t n_out,
                                                     float Dc, float Ds, float dx, float dy, uint32_t key, float sigma_xy, float sigma_t,
                                                     float4* __restrict__ out)
{
    const uint32_t j = (uint32_t)blockIdx.x * kFltTB + threadIdx.x;
    if (j >= n_out) return;
    const uint32_t a = min(ancestors ? ancestors[j] : j, n - 1);
    const float4 st = in[a];
    const Pose2 p = { st.x, st.y, st.z, st.w };
    const float nx = variate(key, j, 0) * sigma_xy, ny = variate(key, j, 1) * sigma_xy, t = variate(key, j, 2) * sigma_t;
    float4 o;
    pose_move(p, dx + nx, dy + ny, &o.z, &o.w);
    const float q = t * t, den = 1.0f + q, nc = (1.0f - q) / den, ns = (t + t) / den;
    const float rc = Dc * nc - Ds * ns, rs = Ds * nc + Dc * ns;
    const float c1 = p.c * rc - p.s * rs, s1 = p.s * rc + p.c * rs;
    const float m = sqrtf(c1 * c1 + s1 * s1);
    o.x = c1 / m;
    o.y = s1 / m;
    out[j] = o;
}

}  // namespace

void filter_tile_sizes(int* scan_tile, int* draws_per_group, int* search_tile)
{
    if (scan_tile) *scan_tile = kFltTile;
    if (draws_per_group) *draws_per_group = kFltDraws;
    if (search_tile) *search_tile = 0;                           // the draws search cum in global memory: no staged stretch
}

void launch_filter_resample(const rr_field_rec* recs, int n, const uint16_t* table, int n_out, const rr_filter_config& f, uint64_t* cum,
                            uint32_t* ancestors, rr_filter_summary* summary, hipStream_t s)
{
    const unsigned un = (unsigned)n, tiles = (un + kFltTile - 1) / kFltTile;
    hipLaunchKernelGGL(k_flt_init, dim3(1), dim3(1), 0, s, summary);
    hipLaunchKernelGGL(k_flt_min, dim3(tiles), dim3(kFltTB), 0, s, recs, un, summary);
    hipLaunchKernelGGL(k_flt_tile, dim3(tiles), dim3(kFltTB), 0, s, recs, un, table, f.quantum, f.n_table, summary, cum);
    hipLaunchKernelGGL(k_flt_tiles, dim3(1), dim3(kFltTB), 0, s, un, summary, cum);
    hipLaunchKernelGGL(k_flt_cum, dim3(tiles), dim3(kFltTB), 0, s, recs, un, table, f.quantum, f.n_table, summary, cum);
    hipLaunchKernelGGL(k_flt_draw, dim3(((unsigned)n_out + kFltDraws - 1) / kFltDraws), dim3(kFltDraws), 0, s, cum, un, (unsigned)n_out, f.phase,
                       summary, ancestors);
}

void launch_filter_move(const float* states_in, int n, const uint32_t* ancestors, int n_out, float Dc, float Ds, float dx, float dy,
                        const rr_filter_config& f, float* states_out, hipStream_t s)
{
    uint32_t key = f.step;                                       // key = mix32(seed ^ mix32(step)), once on the host
    for (int k = 0; k < 2; k++) {
        key ^= key >> 16; key *= 0x7feb352du; key ^= key >> 15; key *= 0x846ca68bu; key ^= key >> 16;
        if (k == 0) key ^= f.seed;
    }
    hipLaunchKernelGGL(k_flt_move, dim3(((unsigned)n_out + kFltTB - 1) / kFltTB), dim3(kFltTB), 0, s, reinterpret_cast<const float4*>(states_in),
                       (unsigned)n, ancestors, (unsigned)n_out, Dc, Ds, dx, dy, key, f.sigma_xy, f.sigma_t,
                       reinterpret_cast<float4*>(states_out));
}

}  // namespace rr
