// rr_shift.hip -- gfx950 kernels that register n mono8 images [H][W] against ONE reference image over a window of pixel shifts
// (rr_shift_images_device; the definitions are in include/radarays_mi355.h): the exact 2-D cross-correlation
// xcorr[dy][dx] = sum over the template window T of x[i][j] r[i + dy][j + dx] for dy, dx in -S..S, the box sums of the reference under
// every shift, and from them the SSE surface, its smallest entry and the scores there.  g = dy + S and f = dx + S index the surface.
//
//   k_shift_box_cols  one thread per reference column: sum r and sum r^2 over the rows of T moved by dy, for g = 0 by a walk down the
//                     column and for every further g by sliding (one row leaves, one enters): col [2S+1][W][2], exact uint64
//   k_shift_box_rows  one workgroup per g: the first window of W - 2S column sums reduced by the workgroup, then slid along the row:
//                     box [2S+1][2S+1][2] = {Sr, Srr}, exact uint64.  Together the two are the issue's k_shift_box: down, then along
//   k_shift_sums      grid (blocks, n_images): Sx and Sxx over T per image, exact uint64 through integer atomics
//   k_shift_gram      one workgroup per (image, tile row of 32 image columns, K-chunk of rows, group of dy).  For one dy the cross
//                     term is a banded Gram product G_dy[a][b] = sum_i x'[i][a] r'[i + dy][b] of the signed values v' = v ^ 0x80
//                     = v - 128 on the matrix cores (__builtin_amdgcn_mfma_i32_32x32x32_i8); element (a, b) belongs to dx = b - a,
//                     and only |b - a| <= S is wanted: the reference columns [a0 - S, a0 + 32 + S), 1 + ceil(S / 16) tiles of 32.
//                     Each of the four waves holds DW values of dy times the band's tiles in i32 accumulators over the workgroup's
//                     whole K-chunk; then element (a, b) goes to the LDS bin of (dy, b - a), and the non-zero bins to the image's
//                     int64 surface with integer atomics
//   k_shift_finish    one workgroup per image: adds the value-domain correction 128 (Sx + Sr[d]) - 16384 N, forms the SSE surface,
//                     finds its smallest entry (smallest index on a tie), counts the entries that attain it, reads its four
//                     neighbours, computes the NCC in f64, writes one rr_shift_record (psnr and sub_* are the host's to fill)
//
// The dy axis.  The workgroup stages the reference strip ONCE per 64 rows, with the rows its group of dy reaches beyond them, as
// [column][84 rows] in LDS; a dy is then a BYTE offset into a column's LDS row.  No unaligned wide LDS read is relied on: the
// operand's 16 bytes are assembled from five aligned 32-bit words with a funnel shift by (offset & 3) bytes, which is the same in
// every lane of a wave because a wave works on one dy at a time.  The LDS row is 21 words, an odd number, so the 32 lanes of a
// half wave read 32 different banks.
//
// Operand layout.  As rr_align.hip: the C/D lane map of the 32x32 MFMA is the same for every dtype -- lane l, register g hold row
// (g & 3) + 8 (g >> 2) + 4 (l >> 5), column l & 31; the rows are the A operand's lanes (image columns), the columns the B operand's
// (reference columns).  The order of the 32 k inside one i8 instruction is NOT relied on: both operands are loaded by ONE rule --
// byte j of lane l is row 32 h + 16 (l >> 5) + j of the strip (plus dy for the reference) -- so whatever k the hardware gives to
// (lane half, byte) it gives to the same image row in both, and a permutation of k does not change a sum over k.
//
// Value domain.  x' outside T is SIGNED zero (byte 0, not 0x80): rows and columns outside T add nothing, and the correction uses
// the true N.  Reference pixels outside the image are signed zero too; they only ever meet an x' of zero.
//
// i32 bounds.  |v'| <= 128.  A tile element over a workgroup's K-chunk of at most kMaxSteps x 64 = 1024 rows: 128^2 x 1024 = 1.7e7.
// A bin (dy, dx) sums at most 32 elements (one per image column of the tile row): 32 x 1.7e7 = 5.4e8 < 2^31.
// Every sum is an integer sum: a call repeats its bits.
// No kernel uses scratch.  LDS, all static: k_shift_gram 20,128 B at S > 32 (reference strip 160 x 84, image strip 32 x 80,
// 8 x 129 bins) and 14,784 B at S <= 32 (96 x 84, 32 x 80, 16 x 65 bins), k_shift_finish 3,080 B, k_shift_box_rows 4,096 B,
// k_shift_box_cols and k_shift_sums none.
#include "../../include/radarays_mi355.h"
#include "rr_device.h"
#include "rr_launch.h"

#include <algorithm>

namespace rr {

namespace {

constexpr int kTile = 32;                                   // MFMA tile edge
constexpr int kStep = 64;                                   // image rows per staged strip: two MFMAs of K = 32
constexpr int kRowX = kStep + 16;                           // bytes per LDS row of the image strip (one column's rows; 16-B aligned)
constexpr int kRowR = 84;                                   // ... of the reference strip: 64 rows + 15 of dy + 3 of the last word, 21 words
constexpr int kTB = 256, kWaves = 4;
constexpr int kMaxSteps = 16;                               // strips per workgroup at most (the i32 bounds above)

using v4i = __attribute__((ext_vector_type(4))) int;
using v16i = __attribute__((ext_vector_type(16))) int;
using u64 = unsigned long long;

// rows [row0, row0 + 4 nq) x columns [col0, col0 + ncol) of img [.][W] as signed bytes into T [ncol][rb]; a pixel outside rows
// [rlo, rhi) or columns [clo, chi) is signed zero and is not read
__device__ inline void stage_rows(const uint8_t* __restrict__ img, int W, int col0, int ncol, int clo, int chi, int row0, int nq, int rlo, int rhi,
                                  uint8_t* T, int rb)
{
    for (int e = threadIdx.x; e < ncol * nq; e += kTB) {
        const int cl = e % ncol, q = e / ncol, c = col0 + cl;
        uint32_t word = 0;
        if (c >= clo && c < chi) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int i = row0 + 4 * q + j;
                if (i >= rlo && i < rhi) word |= (uint32_t)(img[(size_t)i * W + c] ^ 0x80u) << (8 * j);
            }
        }
        *reinterpret_cast<uint32_t*>(T + cl * rb + 4 * q) = word;
    }
}

// bytes [sh, sh + 4) of the eight bytes lo, hi (sh in 0..3): one v_alignbit
__device__ inline int funnel(uint32_t lo, uint32_t hi, int sh) { return (int)(uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh)); }

// grid (tile rows x K-chunks x dy groups, n_images), block 256; surf [n_images][2S+1][2S+1] must be zero before the launch.
// NBT: reference tiles held per dy (nbt <= NBT are in use); DW: values of dy per wave
template <int NBT, int DW>
__global__ void __launch_bounds__(kTB) k_shift_gram(const uint8_t* __restrict__ imgs, const uint8_t* __restrict__ ref, int H, int W, int S, int nbt,
                                                    int steps_per_wg, int n_chunks, int n_dyg, long long* surf)
{
    constexpr int kDyWg = kWaves * DW, kSMax = 16 * (NBT - 1), kBins = kDyWg * (2 * kSMax + 1);
    __shared__ __align__(16) uint8_t Tr[NBT * kTile * kRowR];
    __shared__ __align__(16) uint8_t Tx[kTile * kRowX];
    __shared__ int bins[kBins];
    const int D = 2 * S + 1;
    const int dg = (int)blockIdx.x % n_dyg, kc = ((int)blockIdx.x / n_dyg) % n_chunks, row = (int)blockIdx.x / (n_dyg * n_chunks);
    const int a0 = S + row * kTile, g0 = dg * kDyWg;        // first image column of the tile row (reference column a0 - S), first g
    const uint8_t* img = imgs + (size_t)blockIdx.y * H * W;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);

    for (int d = threadIdx.x; d < kBins; d += kTB) bins[d] = 0;
    v16i acc[DW][NBT];
#pragma unroll
    for (int j = 0; j < DW; j++)
#pragma unroll
        for (int t = 0; t < NBT; t++)
#pragma unroll
            for (int g = 0; g < 16; g++) acc[j][t][g] = 0;

    for (int step = 0; step < steps_per_wg; step++) {
        const int i0 = S + (kc * steps_per_wg + step) * kStep;
        if (i0 >= H - S) break;                             // (the same in every thread)
        __syncthreads();                                    // the strips' readers of the step before are done
        stage_rows(img, W, a0, kTile, S, W - S, i0, kStep / 4, S, H - S, Tx, kRowX);
        stage_rows(ref, W, a0 - S, nbt * kTile, 0, W, i0 + g0 - S, kRowR / 4, 0, H, Tr, kRowR);     // strip row e + k is image row i0 + k + dy
        __syncthreads();
#pragma unroll
        for (int h = 0; h < kStep / 32; h++) {
            const int at = 32 * h + 16 * (lane >> 5);       // ONE rule for both operands (file header)
            const v4i fa = *reinterpret_cast<const v4i*>(Tx + (lane & 31) * kRowX + at);
#pragma unroll
            for (int j = 0; j < DW; j++) {
                const int e = w * DW + j;                   // this wave's dy, as an offset into the group: the same in every lane
                if (g0 + e < D) {
                    const int sh = e & 3;
                    const uint8_t* col = Tr + (lane & 31) * kRowR + at + (e & ~3);
#pragma unroll
                    for (int t = 0; t < NBT; t++) {
                        if (t < nbt) {
                            const uint32_t* p = reinterpret_cast<const uint32_t*>(col + t * kTile * kRowR);
                            const uint32_t w0 = p[0], w1 = p[1], w2 = p[2], w3 = p[3], w4 = p[4];
                            v4i fb;
                            fb[0] = funnel(w0, w1, sh); fb[1] = funnel(w1, w2, sh); fb[2] = funnel(w2, w3, sh); fb[3] = funnel(w3, w4, sh);
                            acc[j][t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa, fb, acc[j][t], 0, 0, 0);
                        }
                    }
                }
            }
        }
    }
    __syncthreads();                                        // bins are zero (and every strip read is done)
#pragma unroll
    for (int j = 0; j < DW; j++) {
        const int e = w * DW + j;
        if (g0 + e < D) {
#pragma unroll
            for (int t = 0; t < NBT; t++) {
                if (t < nbt) {
#pragma unroll
                    for (int g = 0; g < 16; g++) {
                        const int r = (g & 3) + 8 * (g >> 2) + 4 * (lane >> 5);
                        const int f = t * kTile + (lane & 31) - r;          // (a0 - S + column) - (a0 + r) + S = dx + S
                        const int v = acc[j][t][g];
                        if (v && f >= 0 && f < D) atomicAdd(&bins[e * D + f], v);
                    }
                }
            }
        }
    }
    __syncthreads();
    u64* out = reinterpret_cast<u64*>(surf) + (size_t)blockIdx.y * D * D;
    const int n_g = min(kDyWg, D - g0);
    for (int d = threadIdx.x; d < n_g * D; d += kTB) {
        const int v = bins[d];
        if (v) atomicAdd(&out[(size_t)g0 * D + d], (u64)(long long)v);      // two's complement: the sum is the signed sum
    }
}

// grid ceil(W / 64), block 64.  col [2S+1][W][2]
__global__ void __launch_bounds__(64) k_shift_box_cols(const uint8_t* __restrict__ ref, int H, int W, int S, u64* col)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= W) return;
    const int rows = H - 2 * S;
    u64 s1 = 0, s2 = 0;
    for (int i = 0; i < rows; i++) { const u64 v = ref[(size_t)i * W + j]; s1 += v; s2 += v * v; }
    col[2 * (size_t)j] = s1; col[2 * (size_t)j + 1] = s2;
    for (int g = 1; g <= 2 * S; g++) {                      // the window moves down by one row: row g - 1 leaves, row rows + g - 1 enters
        // v^2 - o^2 as (v - o)(v + o), in two's complement: written as "- o * o + v * v" the compiler folds the pair into one
        // v_dot4_u32_u8, which ADDS both squares
        const long long o = ref[(size_t)(g - 1) * W + j], v = ref[(size_t)(rows + g - 1) * W + j];
        s1 += (u64)(v - o); s2 += (u64)((v - o) * (v + o));
        col[2 * ((size_t)g * W + j)] = s1; col[2 * ((size_t)g * W + j) + 1] = s2;
    }
}

// grid 2S+1, block 256.  box [2S+1][2S+1][2]
__global__ void __launch_bounds__(kTB) k_shift_box_rows(const u64* __restrict__ col, int W, int S, u64* box)
{
    __shared__ u64 p1[kTB], p2[kTB];
    const int g = blockIdx.x, t = threadIdx.x, cols = W - 2 * S, D = 2 * S + 1;
    const u64* c = col + 2 * (size_t)g * W;
    u64 s1 = 0, s2 = 0;
    for (int j = t; j < cols; j += kTB) { s1 += c[2 * j]; s2 += c[2 * j + 1]; }
    p1[t] = s1; p2[t] = s2;
    __syncthreads();
    for (int half = kTB / 2; half > 0; half >>= 1) {
        if (t < half) { p1[t] += p1[t + half]; p2[t] += p2[t + half]; }
        __syncthreads();
    }
    if (t == 0) {
        s1 = p1[0]; s2 = p2[0];
        u64* b = box + 2 * (size_t)g * D;
        b[0] = s1; b[1] = s2;
        for (int f = 1; f < D; f++) {                       // the window moves right by one column
            s1 = s1 - c[2 * (f - 1)] + c[2 * (cols + f - 1)];
            s2 = s2 - c[2 * (f - 1) + 1] + c[2 * (cols + f - 1) + 1];
            b[2 * f] = s1; b[2 * f + 1] = s2;
        }
    }
}

// grid (blocks, n_images), block 256.  sums [n_images][2] = {Sx, Sxx} over T, zero before
__global__ void __launch_bounds__(kTB) k_shift_sums(const uint8_t* __restrict__ imgs, int H, int W, int S, u64* sums)
{
    const int k = blockIdx.y, cols = W - 2 * S;
    const size_t n = (size_t)(H - 2 * S) * cols;
    const uint8_t* img = imgs + (size_t)k * H * W;
    u64 s1 = 0, s2 = 0;
    for (size_t p = (size_t)blockIdx.x * kTB + threadIdx.x; p < n; p += (size_t)gridDim.x * kTB) {
        const u64 v = img[(S + p / cols) * W + S + p % cols];
        s1 += v; s2 += v * v;
    }
    for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_down(s1, off); s2 += __shfl_down(s2, off); }
    if ((threadIdx.x & 63) == 0) {
        if (s1) atomicAdd(&sums[2 * k], s1);
        if (s2) atomicAdd(&sums[2 * k + 1], s2);
    }
}

// grid n_images, block 256.  surf [n_images][D][D] holds the signed-domain sums on entry and xcorr on exit; sse [n_images][D][D] or
// null receives the SSE surface; psnr, sub_dy and sub_dx are the host's to fill
__global__ void __launch_bounds__(kTB) k_shift_finish(long long* surf, u64* sse, const u64* __restrict__ sums, const u64* __restrict__ box, int S,
                                                      long long n_px, rr_shift_record* out)
{
    __shared__ u64 best_v[kTB];
    __shared__ int best_d[kTB];
    __shared__ int n_best;
    const int t = threadIdx.x, img = blockIdx.x, D = 2 * S + 1, ND = D * D;
    long long* cv = surf + (size_t)img * ND;
    const u64 sx = sums[2 * img], sxx = sums[2 * img + 1];
    const long long base = 128ll * (long long)sx - 16384ll * n_px;
    u64 bv = 0; int bd = -1;
    for (int d = t; d < ND; d += kTB) {                     // ascending d: a later equal value does not replace an earlier one
        const long long v = cv[d] + base + 128ll * (long long)box[2 * d];
        cv[d] = v;
        const u64 e = sxx + box[2 * d + 1] - 2ull * (u64)v;
        if (sse) sse[(size_t)img * ND + d] = e;
        if (bd < 0 || e < bv) { bv = e; bd = d; }
    }
    best_v[t] = bv; best_d[t] = bd;
    if (t == 0) n_best = 0;
    __syncthreads();                                        // (also: every cv[d] of this image is written)
    for (int half = kTB / 2; half > 0; half >>= 1) {
        if (t < half) {
            const u64 ov = best_v[t + half]; const int od = best_d[t + half];
            if (od >= 0 && (best_d[t] < 0 || ov < best_v[t] || (ov == best_v[t] && od < best_d[t]))) { best_v[t] = ov; best_d[t] = od; }
        }
        __syncthreads();
    }
    const u64 low = best_v[0];
    int cnt = 0;
    for (int d = t; d < ND; d += kTB) cnt += sxx + box[2 * d + 1] - 2ull * (u64)cv[d] == low;
    if (cnt) atomicAdd(&n_best, cnt);
    __syncthreads();
    if (t == 0) {
        const int d = best_d[0], g = d / D, f = d % D;
        const long long top = cv[d];
        const u64 sr = box[2 * d], srr = box[2 * d + 1];
        rr_shift_record m;
        m.dy = g - S; m.dx = f - S; m.n_best = n_best; m.reserved_ = 0;
        m.xcorr = top; m.sse = low;
        m.psnr = 0.0; m.sub_dy = 0.0; m.sub_dx = 0.0;
        // exact int64: N <= 2^23, xcorr, Sxx <= 255^2 N < 2^39, Sx <= 255 N < 2^31
        const long long num = n_px * top - (long long)sx * (long long)sr;
        const long long fx = n_px * (long long)sxx - (long long)sx * (long long)sx, fr = n_px * (long long)srr - (long long)sr * (long long)sr;
        m.ncc = (fx == 0 || fr == 0) ? 0.0 : (double)num / sqrt((double)fx * (double)fr);
        const int nb[4] = { g > 0 ? d - D : -1, g < D - 1 ? d + D : -1, f > 0 ? d - 1 : -1, f < D - 1 ? d + 1 : -1 };
#pragma unroll
        for (int k = 0; k < 4; k++) m.sse_nb[k] = nb[k] < 0 ? ~0ull : sxx + box[2 * nb[k] + 1] - 2ull * (u64)cv[nb[k]];
        m.sum_x = sx; m.sum_xx = sxx; m.sum_r = sr; m.sum_rr = srr;
        out[img] = m;
    }
}

}  // namespace

void launch_shift_box(const uint8_t* ref, int H, int W, int S, unsigned long long* col, unsigned long long* box, hipStream_t s)
{
    hipLaunchKernelGGL(k_shift_box_cols, dim3((unsigned)((W + 63) / 64)), dim3(64), 0, s, ref, H, W, S, col);
    hipLaunchKernelGGL(k_shift_box_rows, dim3((unsigned)(2 * S + 1)), dim3(kTB), 0, s, col, W, S, box);
}

void launch_shift_sums(const uint8_t* imgs, int H, int W, int S, int n_images, unsigned long long* sums, hipStream_t s)
{
    const size_t n = (size_t)(H - 2 * S) * (W - 2 * S);
    const unsigned blocks = (unsigned)std::min<size_t>(64, (n + 4095) / 4096);
    hipLaunchKernelGGL(k_shift_sums, dim3(blocks, (unsigned)n_images), dim3(kTB), 0, s, imgs, H, W, S, sums);
}

void launch_shift_gram(const uint8_t* imgs, const uint8_t* ref, int H, int W, int S, int n_images, long long* surf, hipStream_t s)
{
    const int D = 2 * S + 1, nbt = 1 + (S + 15) / 16;       // reference columns [a0 - S, a0 + 32 + S) in tiles of 32
    const bool wide = S > 32;
    const int dy_wg = wide ? 2 * kWaves : 4 * kWaves, n_dyg = (D + dy_wg - 1) / dy_wg;
    const int rows = (W - 2 * S + kTile - 1) / kTile, steps = (H - 2 * S + kStep - 1) / kStep;
    // strips per workgroup: as many as still leave about 1024 workgroups in the launch, at least 2, at most kMaxSteps
    const long long per = (long long)n_images * rows * n_dyg * steps / 1024;
    const int steps_per_wg = (int)std::min<long long>(kMaxSteps, std::max<long long>(2, per));
    const int n_chunks = (steps + steps_per_wg - 1) / steps_per_wg;
    const dim3 grid((unsigned)(rows * n_chunks * n_dyg), (unsigned)n_images);
    if (wide) hipLaunchKernelGGL((k_shift_gram<5, 2>), grid, dim3(kTB), 0, s, imgs, ref, H, W, S, nbt, steps_per_wg, n_chunks, n_dyg, surf);
    else hipLaunchKernelGGL((k_shift_gram<3, 4>), grid, dim3(kTB), 0, s, imgs, ref, H, W, S, nbt, steps_per_wg, n_chunks, n_dyg, surf);
}

void launch_shift_finish(long long* surf, unsigned long long* sse, const unsigned long long* sums, const unsigned long long* box, int H, int W,
                         int S, int n_images, rr_shift_record* out, hipStream_t s)
{
    hipLaunchKernelGGL(k_shift_finish, dim3((unsigned)n_images), dim3(kTB), 0, s, surf, sse, sums, box, S,
                       (long long)(H - 2 * S) * (W - 2 * S), out);
}

}  // namespace rr
