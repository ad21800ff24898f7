// rr_place.hip -- gfx950 kernels for place recognition (rr_describe_images_device, rr_match_descriptors_device; the definitions are in
// include/radarays_mi355.h): a polar image becomes a descriptor d [R][S] of ring-by-sector means, and n_query descriptors are matched
// against n_db of them over every circular sector shift, xcorr[s] = sum_r sum_j q[r][j] c[r][(j + s) mod S], exactly, on the matrix cores.
//
//   k_place_describe  one workgroup per (ring, image): one pass over the ring's rows, column sums in registers (16-B row loads where the
//                     image base and n_angles are multiples of 16, bytes otherwise), sector sums in LDS (exact uint64), then the floor
//                     divide by the rectangle's pixel count.  No float, no atomics on HBM
//   k_place_rolls     one workgroup per (shift, query): row (q, s) of the A operand [n_query * S][Kpad] is np.roll(q, s, axis=1) flattened,
//                     as signed bytes v' = v ^ 0x80 = v - 128, K = R S padded to a multiple of 64 with SIGNED zero (byte 0); the workgroup
//                     of shift 0 also sums the query: qsums [n_query][2] = {Sq, Sqq}
//   k_place_match     a plain dense int8 GEMM [shifts x K] . [K x candidates] (__builtin_amdgcn_mfma_i32_32x32x32_i8).  One workgroup per
//                     (tile of 32 candidates, group of 4 queries); the 32 candidates' bytes are staged through LDS 256 bytes of K at a time,
//                     by 16-B loads when K % 16 == 0 and the database base is 16-B aligned, by bytes otherwise.  Each of the four waves
//                     owns ONE query's whole shift axis, ceil(S / 32) <= 4 accumulator tiles, over the full K; the A operand comes
//                     straight from the rolls (L2-resident).  xcorr[s] of a (query, candidate) pair for every s therefore sits in one
//                     wave's accumulators: the largest (smallest s on a tie) and the number of shifts that attain it are found down the
//                     C/D rows of a lane, then between the two lanes that hold a column (l and l ^ 32).  No LDS bins, no atomics.
//                     The candidate's Sc and Scc come from the staged bytes, in the signed domain (padding adds nothing):
//                     Sc = Sc' + 128 K, Scc = Scc' + 256 Sc' + 16384 K.  xcorr = xcorr' + 128 (Sq + Sc) - 16384 K over the true K.
//                     Per pair: key = sse << 32 | candidate index, and aux = xcorr | shift << 29 | (n_best - 1) << 36 | Sc << 43
//                     (xcorr <= 255^2 x 8192 < 2^29, shift and n_best - 1 < 2^7, Sc <= 255 x 8192 < 2^21: 64 bits exactly)
//   k_place_topk      the top_k smallest keys of a slice of one query's keys, in ascending order: round r finds the smallest key above
//                     the one of round r - 1.  The keys of a query are unique (each holds its candidate's index), so the result is a set
//                     property and does not depend on the order of evaluation.  Stage one: a workgroup per slice of 4096 candidates;
//                     stage two: one workgroup per query over the slices' winners and the winners carried from earlier database chunks
//   k_place_gather    the aux word of each winner: from this chunk's pairs, or from the carried winners
//   k_place_finish    one thread per (query, rank): the rr_place_match record, NCC in f64 from exact int64 (psnr is the host's to fill)
//
// Operand layout.  As rr_align.hip: the C/D lane map of the 32x32 MFMA -- lane l, register g hold row (g & 3) + 8 (g >> 2) + 4 (l >> 5),
// column l & 31; rows are the A operand's lanes (shifts), columns the B operand's (candidates); g ascending is row ascending.  The order
// of the 32 k inside one i8 instruction is NOT relied on: both operands are loaded by ONE rule -- byte j of lane l is k = 32 h +
// 16 (l >> 5) + j -- so a permutation of k inside the instruction permutes both alike and does not change a sum over k.
// Masks.  A rows s >= S are loaded as zero AND skipped by the reduction; candidates past the end are staged as zero and never written.
// i32 bound.  |v'| <= 128 and K <= 8192: |xcorr'| <= 128^2 x 8192 = 1.3e8 < 2^31; Scc' likewise.
// LDS rows of the staged tile are 272 B apart (68 words): the 16 lanes of a ds_read_b128 group start 4 banks apart, no conflict.
// Every sum is an integer sum: a call repeats its bits.
// No kernel uses scratch.  LDS, all static: k_place_match 8,960 B (32 x 272 staged bytes, 2 x 32 sums), k_place_describe 1,024 B,
// k_place_rolls 32 B, k_place_topk 32 B, k_place_gather and k_place_finish none.
#include "../../include/radarays_mi355.h"
#include "rr_device.h"
#include "rr_launch.h"

#include <algorithm>
#include <climits>

namespace rr {

namespace {

constexpr int kTile = 32;                                   // MFMA tile edge: candidates per workgroup, shifts per accumulator tile
constexpr int kKStep = 256;                                 // bytes of K staged at a time: eight MFMAs of K = 32
constexpr int kRowB = kKStep + 16;                          // bytes per LDS row (one candidate's bytes of the step; 16-B aligned, 68 words)
constexpr int kTB = 256, kWaves = 4;
constexpr int kMaxTiles = 4;                                // ceil(128 / 32) accumulator tiles along the shift axis
constexpr int kSlice = 4096;                                // candidates per stage-one workgroup of the top-k

using v4i = __attribute__((ext_vector_type(4))) int;
using v16i = __attribute__((ext_vector_type(16))) int;
using u64 = unsigned long long;

static_assert(255ll * 255 * 8192 < (1ll << 29) && 255 * 8192 < (1 << 21), "the aux word's fields");

// grid (R, n_images), block 256.  W = 16: 16-B row loads (n_angles % 16 == 0 and a 16-B aligned base); W = 1: bytes
template <int W>
__global__ void __launch_bounds__(kTB) k_place_describe(const uint8_t* __restrict__ imgs, int n_cells, int n_angles, int cell_begin, int cell_end,
                                                        int R, int S, uint8_t* desc)
{
    __shared__ u64 bins[128];
    const int r = blockIdx.x, t = threadIdx.x, L = cell_end - cell_begin;
    const int c0 = cell_begin + (int)((long long)r * L / R), c1 = cell_begin + (int)((long long)(r + 1) * L / R);
    const uint8_t* im = imgs + (size_t)blockIdx.y * n_cells * n_angles;
    if (t < S) bins[t] = 0;
    __syncthreads();
    const int ncg = (n_angles + W - 1) / W;                 // column groups of W columns
    const int across = min(ncg, kTB), nph = kTB / across, ph = t / across;      // the workgroup is `across` column groups by `nph` row phases
    if (ph < nph) {
        for (int cg = t % across; cg < ncg; cg += across) {
            uint32_t sum[W];                                // column sums: at most 255 x 8192
#pragma unroll
            for (int i = 0; i < W; i++) sum[i] = 0;
            for (int row = c0 + ph; row < c1; row += nph) {
                const uint8_t* p = im + (size_t)row * n_angles + (size_t)W * cg;
                if constexpr (W == 16) {
                    const uint4 v = *reinterpret_cast<const uint4*>(p);
                    const uint32_t w4[4] = { v.x, v.y, v.z, v.w };
#pragma unroll
                    for (int i = 0; i < 16; i++) sum[i] += (w4[i >> 2] >> (8 * (i & 3))) & 0xffu;
                } else {
                    sum[0] += *p;
                }
            }
            // column a lies in sector floor(((a + 1) S - 1) / n_angles): the largest j with floor(j n_angles / S) <= a
            const int a = W * cg;
            int j = ((a + 1) * S - 1) / n_angles;
            u64 run = 0;
#pragma unroll
            for (int i = 0; i < W; i++) {
                const int ja = ((a + i + 1) * S - 1) / n_angles;
                if (ja != j) { if (run) atomicAdd(&bins[j], run); run = 0; j = ja; }
                run += sum[i];
            }
            if (run) atomicAdd(&bins[j], run);
        }
    }
    __syncthreads();
    if (t < S) {
        const int a0 = (int)((long long)t * n_angles / S), a1 = (int)((long long)(t + 1) * n_angles / S);
        const u64 count = (u64)(c1 - c0) * (u64)(a1 - a0);  // >= 1: R <= L and S <= n_angles
        desc[((size_t)blockIdx.y * R + r) * S + t] = (uint8_t)(bins[t] / count);
    }
}

// grid (S, n_query), block 256.  rolls [n_query * S][Kpad], qsums [n_query][2]
__global__ void __launch_bounds__(kTB) k_place_rolls(const uint8_t* __restrict__ query, int R, int S, int Kpad, uint8_t* rolls, uint32_t* qsums)
{
    __shared__ uint32_t part[kWaves][2];
    const int s = blockIdx.x, q = blockIdx.y, K = R * S, t = threadIdx.x;
    const uint8_t* qd = query + (size_t)q * K;
    uint32_t* row = reinterpret_cast<uint32_t*>(rolls + ((size_t)q * S + s) * Kpad);
    for (int w = t; w < Kpad / 4; w += kTB) {
        uint32_t word = 0;                                  // k >= K: signed zero
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int k = 4 * w + b;
            if (k < K) {
                const int r = k / S, j = k % S, src = j >= s ? j - s : j - s + S;       // np.roll(q, s, axis=1)[r][j] = q[r][(j - s) mod S]
                word |= (uint32_t)(qd[r * S + src] ^ 0x80u) << (8 * b);
            }
        }
        row[w] = word;
    }
    if (s == 0) {                                           // (the same in every thread)
        uint32_t s1 = 0, s2 = 0;                            // at most 255 x 8192 and 255^2 x 8192
        for (int k = t; k < K; k += kTB) { const uint32_t v = qd[k]; s1 += v; s2 += v * v; }
        for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_down(s1, off); s2 += __shfl_down(s2, off); }
        if ((t & 63) == 0) { part[t >> 6][0] = s1; part[t >> 6][1] = s2; }
        __syncthreads();
        if (t == 0) {
            qsums[2 * q] = part[0][0] + part[1][0] + part[2][0] + part[3][0];
            qsums[2 * q + 1] = part[0][1] + part[1][1] + part[2][1] + part[3][1];
        }
    }
}

// grid tiles of 32 candidates x n_qg groups of 4 queries (the group runs fastest: the groups of one tile follow each other and find the
// tile in L2), block 256.  db: this chunk's n_c candidates, K bytes apart; index_base: the database index of its first.  keys and aux
// [n_query][n_c]; d_sse and d_shift [n_query][n_db] or null, addressed with the database index
template <bool WIDE>
__global__ void __launch_bounds__(kTB) k_place_match(const uint8_t* __restrict__ rolls, const uint32_t* __restrict__ qsums, const uint8_t* __restrict__ db,
                                                     uint32_t n_c, uint32_t index_base, int K, int Kpad, int S, int n_query, int n_qg, u64* keys,
                                                     u64* aux, uint32_t* d_sse, uint16_t* d_shift, size_t n_db)
{
    __shared__ __align__(16) uint8_t Tc[kTile * kRowB];
    __shared__ int sc[kTile], scc[kTile];
    const int qg = (int)(blockIdx.x % (unsigned)n_qg);
    const uint32_t c0 = (blockIdx.x / (unsigned)n_qg) * kTile, n_here = min((uint32_t)kTile, n_c - c0);
    const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int q = qg * kWaves + w, nT = (S + kTile - 1) / kTile;
    const bool live = q < n_query;                          // (the same in every lane of a wave)
    const uint8_t* tile = db + (size_t)c0 * K;

    v16i acc[kMaxTiles];
#pragma unroll
    for (int i = 0; i < kMaxTiles; i++)
#pragma unroll
        for (int g = 0; g < 16; g++) acc[i][g] = 0;
    int s1 = 0, s2 = 0;                                     // signed-domain sums of candidate t >> 3 over this thread's eighth of every step

    for (int k0 = 0; k0 < Kpad; k0 += kKStep) {
        const int kn = min(kKStep, Kpad - k0);              // a multiple of 64
        __syncthreads();                                    // the tile's readers of the step before are done
        if constexpr (WIDE) {                               // K % 16 == 0: a 16-B group lies wholly below K or wholly above
            const int per = kn / 16;
            for (int e = t; e < kTile * per; e += kTB) {
                const int cl = e / per, k = 16 * (e % per);
                uint4 v = make_uint4(0, 0, 0, 0);
                if ((uint32_t)cl < n_here && k0 + k < K) {
                    v = *reinterpret_cast<const uint4*>(tile + (size_t)cl * K + k0 + k);
                    v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
                }
                *reinterpret_cast<uint4*>(Tc + cl * kRowB + k) = v;
            }
        } else {
            const int per = kn / 4;
            for (int e = t; e < kTile * per; e += kTB) {
                const int cl = e / per, k = 4 * (e % per);
                uint32_t word = 0;
                if ((uint32_t)cl < n_here) {
#pragma unroll
                    for (int b = 0; b < 4; b++)
                        if (k0 + k + b < K) word |= (uint32_t)(tile[(size_t)cl * K + k0 + k + b] ^ 0x80u) << (8 * b);
                }
                *reinterpret_cast<uint32_t*>(Tc + cl * kRowB + k) = word;
            }
        }
        __syncthreads();
        {
            const uint32_t* p = reinterpret_cast<const uint32_t*>(Tc + (t >> 3) * kRowB + (t & 7) * (kn / 8));
            for (int i = 0; i < kn / 32; i++) {
                const uint32_t x = p[i];
#pragma unroll
                for (int b = 0; b < 4; b++) { const int v = (int)(int8_t)(x >> (8 * b)); s1 += v; s2 += v * v; }
            }
        }
        if (live) {
            for (int h = 0; h < kn / 32; h++) {
                const int at = 32 * h + 16 * (lane >> 5);   // ONE rule for both operands (file header)
                const v4i fb = *reinterpret_cast<const v4i*>(Tc + (lane & 31) * kRowB + at);
#pragma unroll
                for (int i = 0; i < kMaxTiles; i++) {
                    if (i < nT) {
                        const int row = i * kTile + (lane & 31);
                        v4i fa = { 0, 0, 0, 0 };
                        if (row < S) fa = *reinterpret_cast<const v4i*>(rolls + ((size_t)q * S + row) * Kpad + k0 + at);
                        acc[i] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb, acc[i], 0, 0, 0);
                    }
                }
            }
        }
    }
    for (int off = 1; off < 8; off <<= 1) { s1 += __shfl_xor(s1, off); s2 += __shfl_xor(s2, off); }
    if ((t & 7) == 0) { sc[t >> 3] = s1 + 128 * K; scc[t >> 3] = s2 + 256 * s1 + 16384 * K; }
    __syncthreads();
    if (!live) return;

    int bv = INT_MIN, bs = 0, cnt = 0;                      // ascending s within a lane: a later equal value does not replace an earlier one
#pragma unroll
    for (int i = 0; i < kMaxTiles; i++) {
        if (i < nT) {
#pragma unroll
            for (int g = 0; g < 16; g++) {
                const int s = i * kTile + (g & 3) + 8 * (g >> 2) + 4 * (lane >> 5), v = acc[i][g];
                if (s < S) {
                    if (v > bv) { bv = v; bs = s; cnt = 1; }
                    else if (v == bv) cnt++;
                }
            }
        }
    }
    const int ov = __shfl_xor(bv, 32), os = __shfl_xor(bs, 32), oc = __shfl_xor(cnt, 32);    // the other half of this column's rows
    if (ov > bv) { bs = os; cnt = oc; }
    else if (ov == bv) { bs = min(bs, os); cnt += oc; }
    bv = max(bv, ov);
    const uint32_t c = c0 + (uint32_t)lane;
    if (lane < kTile && c < n_c) {
        const int Sc = sc[lane];
        const int xc = (int)((long long)bv + 128ll * ((long long)qsums[2 * q] + Sc) - 16384ll * K);
        const uint32_t sse = qsums[2 * q + 1] + (uint32_t)scc[lane] - 2u * (uint32_t)xc;
        const uint32_t index = index_base + c;
        keys[(size_t)q * n_c + c] = ((u64)sse << 32) | index;
        aux[(size_t)q * n_c + c] = (u64)(uint32_t)xc | ((u64)bs << 29) | ((u64)(cnt - 1) << 36) | ((u64)Sc << 43);
        if (d_sse) d_sse[(size_t)q * n_db + index] = sse;
        if (d_shift) d_shift[(size_t)q * n_db + index] = (uint16_t)bs;
    }
}

// grid (n_slices, n_query), block 256.  in [n_query][n_in]: this workgroup takes [x slice, (x + 1) slice); extra [n_query][top_k] or null
// joins every workgroup's keys; out [n_query][n_slices][top_k] ascending, ~0 where the keys run out (a key is below ~0: sse < 2^31)
__global__ void __launch_bounds__(kTB) k_place_topk(const u64* __restrict__ in, size_t n_in, size_t slice, const u64* __restrict__ extra, int top_k, u64* out)
{
    __shared__ u64 part[kWaves];
    const int t = threadIdx.x;
    const size_t q = blockIdx.y, lo = (size_t)blockIdx.x * slice, hi = min(n_in, lo + slice);
    const u64* kq = in + q * n_in;
    u64* o = out + (q * gridDim.x + blockIdx.x) * (size_t)top_k;
    u64 prev = 0;
    for (int r = 0; r < top_k; r++) {
        u64 m = ~0ull;
        for (size_t i = lo + t; i < hi; i += kTB) { const u64 v = kq[i]; if ((r == 0 || v > prev) && v < m) m = v; }
        if (extra && t < top_k) { const u64 v = extra[q * top_k + t]; if ((r == 0 || v > prev) && v < m) m = v; }
        for (int off = 32; off > 0; off >>= 1) { const u64 v = __shfl_xor(m, off); m = v < m ? v : m; }
        __syncthreads();                                    // part's readers of the round before are done
        if ((t & 63) == 0) part[t >> 6] = m;
        __syncthreads();
        m = min(min(part[0], part[1]), min(part[2], part[3]));
        if (t == 0) o[r] = m;
        prev = m;                                           // (~0 once the keys have run out: nothing is above it, every later round gives ~0)
    }
}

// n_query * top_k threads.  win [n_query][top_k]: the winners so far; their aux words come from this chunk's pairs [n_query][n_c] (index
// >= index_base) or from the winners carried in, old_keys / old_aux [n_query][top_k]
__global__ void __launch_bounds__(kTB) k_place_gather(const u64* __restrict__ win, const u64* __restrict__ aux, size_t n_c, uint32_t index_base,
                                                      const u64* __restrict__ old_keys, const u64* __restrict__ old_aux, int n_query, int top_k, u64* win_aux)
{
    const int e = blockIdx.x * kTB + threadIdx.x;
    if (e >= n_query * top_k) return;
    const int q = e / top_k;
    const u64 key = win[e];
    u64 a = 0;
    if (key != ~0ull) {
        const uint32_t index = (uint32_t)key;
        if (index >= index_base) a = aux[(size_t)q * n_c + (index - index_base)];
        else
            for (int j = 0; j < top_k; j++)
                if (old_keys[q * top_k + j] == key) a = old_aux[q * top_k + j];
    }
    win_aux[e] = a;
}

// n_query * top_k threads.  psnr is the host's to fill from sse (the expression rr_score_images_device uses)
__global__ void __launch_bounds__(kTB) k_place_finish(const u64* __restrict__ win, const u64* __restrict__ win_aux, const uint32_t* __restrict__ qsums,
                                                      int n_query, int top_k, long long K, rr_place_match* out)
{
    const int e = blockIdx.x * kTB + threadIdx.x;
    if (e >= n_query * top_k) return;
    const int q = e / top_k;
    const u64 key = win[e], a = win_aux[e];
    rr_place_match m;
    m.index = (uint32_t)key; m.sse = (uint32_t)(key >> 32);
    m.shift = (int)((a >> 29) & 127); m.n_best = (uint32_t)((a >> 36) & 127) + 1;
    const long long xc = (long long)(a & ((1ull << 29) - 1)), sc = (long long)(a >> 43), sq = qsums[2 * q], sqq = qsums[2 * q + 1];
    const long long scc = (long long)m.sse - sqq + 2 * xc;
    m.xcorr = xc;
    // exact int64: K <= 2^13, xcorr, Sqq, Scc < 2^29, Sq, Sc < 2^21
    const long long num = K * xc - sq * sc, fq = K * sqq - sq * sq, fc = K * scc - sc * sc;
    m.ncc = (fq == 0 || fc == 0) ? 0.0 : (double)num / sqrt((double)fq * (double)fc);
    m.psnr = 0.0;
    out[e] = m;
}

}  // namespace

void launch_place_describe(const uint8_t* imgs, int n_images, int n_cells, int n_angles, const rr_place_config& p, uint8_t* desc, hipStream_t s)
{
    const dim3 grid((unsigned)p.n_rings, (unsigned)n_images);
    const bool wide = n_angles % 16 == 0 && reinterpret_cast<uintptr_t>(imgs) % 16 == 0;
    if (wide) hipLaunchKernelGGL(k_place_describe<16>, grid, dim3(kTB), 0, s, imgs, n_cells, n_angles, p.cell_begin, p.cell_end, p.n_rings, p.n_sectors, desc);
    else hipLaunchKernelGGL(k_place_describe<1>, grid, dim3(kTB), 0, s, imgs, n_cells, n_angles, p.cell_begin, p.cell_end, p.n_rings, p.n_sectors, desc);
}

int place_kpad(int n_rings, int n_sectors) { return (n_rings * n_sectors + 63) / 64 * 64; }

size_t place_slices(size_t n_candidates) { return (n_candidates + kSlice - 1) / kSlice; }

void launch_place_rolls(const uint8_t* query, int n_query, int n_rings, int n_sectors, uint8_t* rolls, uint32_t* qsums, hipStream_t s)
{
    hipLaunchKernelGGL(k_place_rolls, dim3((unsigned)n_sectors, (unsigned)n_query), dim3(kTB), 0, s, query, n_rings, n_sectors,
                       place_kpad(n_rings, n_sectors), rolls, qsums);
}

void launch_place_match(const uint8_t* rolls, const uint32_t* qsums, int n_query, const uint8_t* db, size_t n_candidates, size_t index_base,
                        int n_rings, int n_sectors, unsigned long long* keys, unsigned long long* aux, uint32_t* d_sse, uint16_t* d_shift, size_t n_db,
                        hipStream_t s)
{
    const int K = n_rings * n_sectors, n_qg = (n_query + kWaves - 1) / kWaves;
    const dim3 grid((unsigned)((n_candidates + kTile - 1) / kTile * (size_t)n_qg));
    const bool wide = K % 16 == 0 && reinterpret_cast<uintptr_t>(db) % 16 == 0;
    if (wide) hipLaunchKernelGGL(k_place_match<true>, grid, dim3(kTB), 0, s, rolls, qsums, db, (uint32_t)n_candidates, (uint32_t)index_base, K,
                                 place_kpad(n_rings, n_sectors), n_sectors, n_query, n_qg, keys, aux, d_sse, d_shift, n_db);
    else hipLaunchKernelGGL(k_place_match<false>, grid, dim3(kTB), 0, s, rolls, qsums, db, (uint32_t)n_candidates, (uint32_t)index_base, K,
                            place_kpad(n_rings, n_sectors), n_sectors, n_query, n_qg, keys, aux, d_sse, d_shift, n_db);
}

void launch_place_topk(const unsigned long long* keys, const unsigned long long* aux, int n_query, size_t n_candidates, size_t index_base, int top_k,
                       unsigned long long* part, const unsigned long long* old_keys, const unsigned long long* old_aux, unsigned long long* win,
                       unsigned long long* win_aux, hipStream_t s)
{
    const size_t n_slices = place_slices(n_candidates);
    hipLaunchKernelGGL(k_place_topk, dim3((unsigned)n_slices, (unsigned)n_query), dim3(kTB), 0, s, keys, n_candidates, (size_t)kSlice, nullptr, top_k, part);
    hipLaunchKernelGGL(k_place_topk, dim3(1, (unsigned)n_query), dim3(kTB), 0, s, part, n_slices * top_k, n_slices * top_k, old_keys, top_k, win);
    hipLaunchKernelGGL(k_place_gather, dim3((unsigned)((n_query * top_k + kTB - 1) / kTB)), dim3(kTB), 0, s, win, aux, n_candidates, (uint32_t)index_base,
                       old_keys, old_aux, n_query, top_k, win_aux);
}

void launch_place_finish(const unsigned long long* win, const unsigned long long* win_aux, const uint32_t* qsums, int n_query, int top_k, int n_rings,
                         int n_sectors, rr_place_match* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_place_finish, dim3((unsigned)((n_query * top_k + kTB - 1) / kTB)), dim3(kTB), 0, s, win, win_aux, qsums, n_query, top_k,
                       (long long)n_rings * n_sectors, out);
}

}  // namespace rr
