// rr_align.hip -- gfx950 kernels that register n mono8 images against ONE reference image along the azimuth axis
// (rr_align_images_device; the definitions are in include/radarays_mi355.h): the exact circular cross-correlation
// xcorr[s] = sum x[c][a] r[c][(a + s) mod n_angles] for every s, and from it the best shift with its SSE, PSNR and NCC.
//
//   k_align_sums    grid (blocks, n_images + 1): sum v and sum v^2 over the cell window, per image and (last row) for the reference,
//                   exact uint64 through integer atomics
//   k_align_gram    one workgroup per (image, tile row of 32 image azimuths, K-chunk of cells) over ALL reference azimuths (16 tiles,
//                   512 azimuths, per column group: one group up to n_angles = 512).  The Gram product G[a][b] = sum_c x'[c][a] r'[c][b]
//                   of the signed values v' = v ^ 0x80 = v - 128 on the matrix cores (__builtin_amdgcn_mfma_i32_32x32x32_i8), each of
//                   the four waves holding up to four 32 x 32 i32 tiles over the workgroup's whole K-chunk; then element (a, b) goes
//                   to the LDS bin of its diagonal b - a, and the non-zero bins to the image's int64 curve at (b - a) mod n_angles
//                   with integer atomics
//   k_align_finish  one workgroup per image: adds the value-domain correction 128 (Sx + Sr) - 16384 N to the curve, finds the
//                   largest xcorr (smallest s on a tie), counts the shifts that attain it, writes one rr_align_record
//
// Why (image, tile row, K-chunk): the accumulators stay in registers over the whole K-chunk, so the diagonal reduction (LDS atomics,
// the expensive part per tile) is paid once per workgroup and not once per staged strip; and one image at 3424 x 400 is still 13 tile
// rows x 27 chunks = 351 workgroups, which fills the chip.  The price is that a tile row re-reads the reference strip, from L2.
//
// Operand layout.  The C/D lane map of the 32x32 MFMA is the same for every dtype: lane l, register g hold row (g & 3) + 8 (g >> 2)
// + 4 (l >> 5), column l & 31; the rows are the A operand's lanes (image azimuths), the columns the B operand's (reference azimuths).
// The order of the 32 k inside one i8 instruction is NOT relied on: both operands are loaded by ONE rule -- byte j of lane l is cell
// 32 h + 16 (l >> 5) + j of the strip, for A and for B alike, from the same LDS layout -- so whatever k the hardware gives to
// (lane half, byte) it gives to the same cell in both, and a permutation of k does not change a sum over k.
//
// Transposed staging.  An operand is 16 consecutive cells of one azimuth column, n_angles bytes apart in the image.  A strip of 64
// cells is read with lanes along the azimuth (coalesced bytes, any alignment of the bases), four cells of one azimuth are packed
// into a word and written to an LDS image [azimuth][64 cells + 16 B pad]; an operand is then one 16-B LDS read.  Cells past the
// window and azimuths past n_angles are SIGNED zero (byte 0, not 0x80): they add nothing, and the correction uses the true N.
//
// i32 bounds.  |v'| <= 128.  A tile element over a workgroup's K-chunk of at most kMaxSteps x 64 = 1024 cells: 128^2 x 1024 = 1.7e7.
// A diagonal bin sums at most 32 elements (one per row of the tile row; a diagonal crosses each row once): 32 x 1.7e7 = 5.4e8 < 2^31.
// Every sum is an integer sum: a call repeats its bits.
// No kernel uses scratch.  LDS, all static: k_align_gram 45,692 B (reference strip 512 x 80, image strip 32 x 80, 543 bins),
// k_align_finish 3,080 B, k_align_sums none.
#include "../../include/radarays_mi355.h"
#include "rr_device.h"
#include "rr_launch.h"

#include <algorithm>

namespace rr {

namespace {

constexpr int kTile = 32;                                   // MFMA tile edge
constexpr int kStep = 64;                                   // cells per staged strip: two MFMAs of K = 32
constexpr int kRowB = kStep + 16;                           // bytes per LDS row (one azimuth's cells of the strip, padded; 16-B aligned)
constexpr int kTB = 256, kWaves = 4;
constexpr int kTPW = 4;                                     // reference tiles per wave
constexpr int kColTiles = kWaves * kTPW;                    // reference tiles per workgroup (column group)
constexpr int kDiag = kColTiles * kTile + kTile - 1;        // diagonals b - a of a tile row against a column group
constexpr int kMaxSteps = 16;                               // strips per workgroup at most (the i32 bounds above)

using v4i = __attribute__((ext_vector_type(4))) int;
using v16i = __attribute__((ext_vector_type(16))) int;

// cells [cell0, cell0 + 64) x azimuths [ang0, ang0 + n_ang) of img as signed bytes into T [n_ang][kRowB]
__device__ inline void stage_strip(const uint8_t* __restrict__ img, int n_angles, int ang0, int n_ang, int cell0, int cell_end, uint8_t* T)
{
    for (int e = threadIdx.x; e < n_ang * (kStep / 4); e += kTB) {
        const int al = e % n_ang, q = e / n_ang, a = ang0 + al;
        uint32_t word = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int c = cell0 + 4 * q + j;
            if (a < n_angles && c < cell_end) word |= (uint32_t)(img[(size_t)c * n_angles + a] ^ 0x80u) << (8 * j);
        }
        *reinterpret_cast<uint32_t*>(T + al * kRowB + 4 * q) = word;
    }
}

// grid (tile rows x column groups x K-chunks, n_images), block 256; curve [n_images][n_angles] must be zero before the launch
__global__ void __launch_bounds__(kTB) k_align_gram(const uint8_t* __restrict__ imgs, const uint8_t* __restrict__ ref, int n_cells, int n_angles,
                                                    int cell_begin, int cell_end, int steps_per_wg, int n_chunks, int col_groups,
                                                    long long* curve)
{
    __shared__ __align__(16) uint8_t Tr[kColTiles * kTile * kRowB];
    __shared__ __align__(16) uint8_t Tx[kTile * kRowB];
    __shared__ int bins[kDiag];
    const int tiles = (n_angles + kTile - 1) / kTile;
    const int kc = (int)blockIdx.x % n_chunks, cg = ((int)blockIdx.x / n_chunks) % col_groups, row = (int)blockIdx.x / (n_chunks * col_groups);
    const int a0 = row * kTile, bt0 = cg * kColTiles, nbt = min(kColTiles, tiles - bt0);
    const uint8_t* img = imgs + (size_t)blockIdx.y * n_cells * n_angles;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;

    for (int d = threadIdx.x; d < kDiag; d += kTB) bins[d] = 0;
    v16i acc[kTPW];
#pragma unroll
    for (int i = 0; i < kTPW; i++)
#pragma unroll
        for (int g = 0; g < 16; g++) acc[i][g] = 0;

    for (int step = 0; step < steps_per_wg; step++) {
        const int cell0 = cell_begin + (kc * steps_per_wg + step) * kStep;
        if (cell0 >= cell_end) break;                       // (the same in every thread)
        __syncthreads();                                    // the strips' readers of the step before are done
        stage_strip(img, n_angles, a0, kTile, cell0, cell_end, Tx);
        stage_strip(ref, n_angles, bt0 * kTile, nbt * kTile, cell0, cell_end, Tr);
        __syncthreads();
#pragma unroll
        for (int h = 0; h < kStep / 32; h++) {
            const int at = 32 * h + 16 * (lane >> 5);       // ONE rule for both operands (file header)
            const v4i fa = *reinterpret_cast<const v4i*>(Tx + (lane & 31) * kRowB + at);
#pragma unroll
            for (int i = 0; i < kTPW; i++) {
                const int t = w + kWaves * i;
                if (t < nbt) {
                    const v4i fb = *reinterpret_cast<const v4i*>(Tr + (t * kTile + (lane & 31)) * kRowB + at);
                    acc[i] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb, acc[i], 0, 0, 0);
                }
            }
        }
    }
    __syncthreads();                                        // bins are zero (and every strip read is done)
#pragma unroll
    for (int i = 0; i < kTPW; i++) {
        const int t = w + kWaves * i;
        if (t < nbt) {
#pragma unroll
            for (int g = 0; g < 16; g++) {
                const int r = (g & 3) + 8 * (g >> 2) + 4 * (lane >> 5), col = t * kTile + (lane & 31);
                const int v = acc[i][g];
                if (v) atomicAdd(&bins[col - r + kTile - 1], v);
            }
        }
    }
    __syncthreads();
    unsigned long long* out = reinterpret_cast<unsigned long long*>(curve) + (size_t)blockIdx.y * n_angles;
    for (int d = threadIdx.x; d < kDiag; d += kTB) {
        const int v = bins[d];
        if (v) {
            const int diff = bt0 * kTile + d - (kTile - 1) - a0;             // b - a, in (-n_angles - 32, n_angles + 32)
            const int s = ((diff % n_angles) + n_angles) % n_angles;
            atomicAdd(&out[s], (unsigned long long)(long long)v);           // two's complement: the sum is the signed sum
        }
    }
}

// grid (blocks, n_images + 1), block 256: row n_images is the reference.  sums [n_images + 1][2] = {sum v, sum v^2}, zero before
__global__ void __launch_bounds__(kTB) k_align_sums(const uint8_t* __restrict__ imgs, const uint8_t* __restrict__ ref, size_t npx, size_t lo,
                                                    size_t hi, int n_images, unsigned long long* sums)
{
    const int k = blockIdx.y;
    const uint8_t* img = k < n_images ? imgs + (size_t)k * npx : ref;
    unsigned long long s1 = 0, s2 = 0;
    for (size_t i = lo + (size_t)blockIdx.x * kTB + threadIdx.x; i < hi; i += (size_t)gridDim.x * kTB) {
        const unsigned long long v = img[i];
        s1 += v; s2 += v * v;
    }
    for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_down(s1, off); s2 += __shfl_down(s2, off); }
    if ((threadIdx.x & 63) == 0) {
        if (s1) atomicAdd(&sums[2 * k], s1);
        if (s2) atomicAdd(&sums[2 * k + 1], s2);
    }
}

// grid n_images, block 256.  curve [n_images][n_angles] holds the signed-domain sums on entry and xcorr on exit; psnr is the
// host's to fill from sse (the expression rr_score_images_device uses)
__global__ void __launch_bounds__(kTB) k_align_finish(long long* curve, const unsigned long long* __restrict__ sums, int n_images, int n_angles,
                                                      long long n_px, rr_align_record* out)
{
    __shared__ long long best_v[kTB];
    __shared__ int best_s[kTB];
    __shared__ int n_best;
    const int t = threadIdx.x, img = blockIdx.x;
    long long* cv = curve + (size_t)img * n_angles;
    const unsigned long long sx = sums[2 * img], sxx = sums[2 * img + 1], sr = sums[2 * n_images], srr = sums[2 * n_images + 1];
    const long long corr = 128ll * (long long)(sx + sr) - 16384ll * n_px;
    long long bv = 0; int bs = -1;
    for (int s = t; s < n_angles; s += kTB) {               // ascending s: a later equal value does not replace an earlier one
        const long long v = cv[s] + corr;
        cv[s] = v;
        if (bs < 0 || v > bv) { bv = v; bs = s; }
    }
    best_v[t] = bv; best_s[t] = bs;
    if (t == 0) n_best = 0;
    __syncthreads();
    for (int half = kTB / 2; half > 0; half >>= 1) {
        if (t < half) {
            const long long ov = best_v[t + half]; const int os = best_s[t + half];
            if (os >= 0 && (best_s[t] < 0 || ov > best_v[t] || (ov == best_v[t] && os < best_s[t]))) { best_v[t] = ov; best_s[t] = os; }
        }
        __syncthreads();
    }
    const long long top = best_v[0];
    int cnt = 0;
    for (int s = t; s < n_angles; s += kTB) cnt += cv[s] == top;      // (this thread's own writes)
    if (cnt) atomicAdd(&n_best, cnt);
    __syncthreads();
    if (t == 0) {
        rr_align_record m;
        m.shift = best_s[0]; m.n_best = n_best; m.xcorr = top;
        m.sse = sxx + srr - 2ull * (unsigned long long)top;
        m.psnr = 0.0;
        // exact int64: N <= 2^23, xcorr, Sxx <= 255^2 N < 2^39, Sx <= 255 N < 2^31
        const long long num = n_px * top - (long long)sx * (long long)sr;
        const long long fx = n_px * (long long)sxx - (long long)sx * (long long)sx, fr = n_px * (long long)srr - (long long)sr * (long long)sr;
        m.ncc = (fx == 0 || fr == 0) ? 0.0 : (double)num / sqrt((double)fx * (double)fr);
        m.sum_x = sx; m.sum_xx = sxx; m.sum_r = sr; m.sum_rr = srr;
        out[img] = m;
    }
}

}  // namespace

void launch_align_sums(const uint8_t* imgs, const uint8_t* ref, int n_cells, int n_angles, int cell_begin, int cell_end, int n_images,
                       unsigned long long* sums, hipStream_t s)
{
    const size_t npx = (size_t)n_cells * n_angles, lo = (size_t)cell_begin * n_angles, hi = (size_t)cell_end * n_angles;
    const unsigned blocks = (unsigned)std::min<size_t>(64, (hi - lo + 4095) / 4096);
    hipLaunchKernelGGL(k_align_sums, dim3(blocks, (unsigned)n_images + 1), dim3(kTB), 0, s, imgs, ref, npx, lo, hi, n_images, sums);
}

void launch_align_gram(const uint8_t* imgs, const uint8_t* ref, int n_cells, int n_angles, int cell_begin, int cell_end, int n_images,
                       long long* curve, hipStream_t s)
{
    const int tiles = (n_angles + kTile - 1) / kTile, col_groups = (tiles + kColTiles - 1) / kColTiles;
    const int steps = (cell_end - cell_begin + kStep - 1) / kStep;
    // strips per workgroup: as many as still leave about 1024 workgroups in the launch, at least 2, at most kMaxSteps
    const long long per = (long long)n_images * tiles * col_groups * steps / 1024;
    const int steps_per_wg = (int)std::min<long long>(kMaxSteps, std::max<long long>(2, per));
    const int n_chunks = (steps + steps_per_wg - 1) / steps_per_wg;
    hipLaunchKernelGGL(k_align_gram, dim3((unsigned)(tiles * col_groups * n_chunks), (unsigned)n_images), dim3(kTB), 0, s,
                       imgs, ref, n_cells, n_angles, cell_begin, cell_end, steps_per_wg, n_chunks, col_groups, curve);
}

void launch_align_finish(long long* curve, const unsigned long long* sums, int n_images, int n_angles, int cell_begin, int cell_end,
                         rr_align_record* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_align_finish, dim3((unsigned)n_images), dim3(kTB), 0, s, curve, sums, n_images, n_angles,
                       (long long)(cell_end - cell_begin) * n_angles, out);
}

}  // namespace rr
