// rr_metrics.hip -- gfx950 kernels that compare n mono8 images with ONE reference image (rr_compare_images_device; the
// definitions are in include/radarays_mi355.h): SSIM and the joint histogram with its entropies.  The PSNR part is k_score.
//
//   k_joint_hist<true>   one workgroup per (strip of 65,520 pixels, image): a workgroup-private 256 x 256 histogram of packed
//                        16-bit counts in LDS (128 KB; a strip is shorter than 2^16 pixels, so a half-word cannot carry), flushed
//                        to the image's uint32 histogram with integer atomics on its non-zero words
//   k_joint_hist<false>  the same walk with global integer atomics (RR_METRICS_HIST=1: 24-32x slower, DESIGN_EXPERIMENTS.md)
//   k_ssim               one workgroup per (tile of 32 x 64 window positions, image): both tiles with their halo in LDS, the five
//                        window sums as exact integers (horizontal sums of every tile row, then a running sum down each column),
//                        S per position in f64, one f64 partial per workgroup at [image][block]
//   k_metrics_finish     one workgroup per image: marginals and the three entropy sums of the histogram, the SSIM partials,
//                        one rr_image_metrics record
//
// In both histogram shapes a lane reads 16 neighbouring pixels (16-B loads where the two bases allow, bytes otherwise) and
// merges runs of equal (image, reference) pairs before it issues an atomic: a radar image is mostly dark, and one atomic per
// pixel would queue on a handful of bins.  Every sum is an integer sum or an f64 sum in a fixed order: a call repeats its bits.
// No kernel uses scratch; k_ssim's LDS is dynamic (at most 54 KB), k_joint_hist<true>'s static (128 KB), the rest below 2 KB.
#include "../../include/radarays_mi355.h"
#include "rr_device.h"
#include "rr_launch.h"

#include <algorithm>

namespace rr {

namespace {

constexpr int kHistStrip = 65520;       // pixels per workgroup: a multiple of 16 below 2^16
constexpr int kHistTB = 1024;
constexpr int kSsimTW = 64, kSsimTH = 32, kSsimTB = 256;
constexpr int kSsimRows = kSsimTH / (kSsimTB / kSsimTW);      // window positions a thread walks down its column

// count pairs (key = image value * 256 + reference value) into h: LDS words of two 16-bit counts, or uint32 bins in HBM
template <bool LDS>
__device__ inline void hist_add(uint32_t* h, uint32_t key, uint32_t count)
{
    if (LDS) atomicAdd(&h[key >> 1], count << ((key & 1u) * 16u));
    else atomicAdd(&h[key], count);
}

// pixels [lo, hi) of one image against the reference, lanes of `nthreads` threads striding over groups of 16 pixels
template <bool LDS>
__device__ inline void hist_walk(const uint8_t* img, const uint8_t* ref, size_t lo, size_t hi, uint32_t* h, size_t tid, size_t nthreads)
{
    const bool aligned = ((reinterpret_cast<uintptr_t>(img + lo) | reinterpret_cast<uintptr_t>(ref + lo)) & 15u) == 0;
    const size_t n16 = aligned ? (hi - lo) / 16 : 0;
    for (size_t i = tid; i < n16; i += nthreads) {
        const uint4 a = reinterpret_cast<const uint4*>(img + lo)[i], b = reinterpret_cast<const uint4*>(ref + lo)[i];
        const uint32_t aw[4] = { a.x, a.y, a.z, a.w }, bw[4] = { b.x, b.y, b.z, b.w };
        uint32_t run_key = (((aw[0]) & 0xFFu) << 8) | (bw[0] & 0xFFu), run = 0;
#pragma unroll
        for (int w = 0; w < 4; w++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t key = (((aw[w] >> (8 * k)) & 0xFFu) << 8) | ((bw[w] >> (8 * k)) & 0xFFu);
                if (key != run_key) { hist_add<LDS>(h, run_key, run); run_key = key; run = 0; }
                run++;
            }
        hist_add<LDS>(h, run_key, run);
    }
    for (size_t i = lo + n16 * 16 + tid; i < hi; i += nthreads) hist_add<LDS>(h, ((uint32_t)img[i] << 8) | ref[i], 1u);
}

// grid (strips, n_images); hist [n_images][256][256] must be zero before the launch
template <bool LDS>
__global__ void __launch_bounds__(LDS ? kHistTB : 256) k_joint_hist(const uint8_t* __restrict__ imgs, const uint8_t* __restrict__ ref,
                                                                     size_t npx, uint32_t* hist)
{
    const uint8_t* img = imgs + (size_t)blockIdx.y * npx;
    uint32_t* H = hist + (size_t)blockIdx.y * 65536;
    if constexpr (LDS) {
        __shared__ uint32_t h[32768];
        for (int w = threadIdx.x; w < 32768; w += kHistTB) h[w] = 0;
        __syncthreads();
        const size_t lo = (size_t)blockIdx.x * kHistStrip;
        hist_walk<true>(img, ref, lo, lo + kHistStrip < npx ? lo + kHistStrip : npx, h, threadIdx.x, kHistTB);
        __syncthreads();
        for (int w = threadIdx.x; w < 32768; w += kHistTB) {
            const uint32_t v = h[w];
            if (v & 0xFFFFu) atomicAdd(&H[2 * w], v & 0xFFFFu);
            if (v >> 16) atomicAdd(&H[2 * w + 1], v >> 16);
        }
    } else {
        // strips as above, so that the 16-B groups start where they start there
        const size_t lo = (size_t)blockIdx.x * kHistStrip;
        hist_walk<false>(img, ref, lo, lo + kHistStrip < npx ? lo + kHistStrip : npx, H, threadIdx.x, blockDim.x);
    }
}

// f64 sum over the workgroup (256 threads) in a fixed order, the same value in every thread
__device__ inline double block_sum(double v, double* part)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    __syncthreads();                    // earlier readers of `part` are done
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((part[0] + part[1]) + part[2]) + part[3];
}

// LDS of an SSIM workgroup: the horizontal sums [TH + w - 1][TW] (16 B each), then both tiles [TH + w - 1][TW + w - 1]
size_t ssim_lds(int w)
{
    const size_t in_h = kSsimTH + w - 1, in_w = kSsimTW + w - 1;
    return in_h * kSsimTW * 16 + 2 * ((in_h * in_w + 15) & ~(size_t)15);
}

// grid (tiles, n_images), block 256.  Window position (i, j), i < n_cells - w + 1, j < n_angles - w + 1, covers image rows
// i .. i + w - 1 and columns j .. j + w - 1 (skimage's crop of (w - 1) / 2 on every side, in the window's corner coordinates)
__global__ void __launch_bounds__(kSsimTB) k_ssim(const uint8_t* __restrict__ imgs, const uint8_t* __restrict__ ref, int n_cells,
                                                  int n_angles, int w, int tiles_x, double* partial)
{
    extern __shared__ __align__(16) uint8_t smem[];
    __shared__ double s_part[4];
    const int in_h = kSsimTH + w - 1, in_w = kSsimTW + w - 1;
    uint4* hs = reinterpret_cast<uint4*>(smem);                          // {sum x | sum y << 16, sum x^2, sum y^2, sum xy}
    uint8_t* tx = smem + (size_t)in_h * kSsimTW * 16;
    uint8_t* ty = tx + (((size_t)in_h * in_w + 15) & ~(size_t)15);
    const uint8_t* img = imgs + (size_t)blockIdx.y * n_cells * n_angles;
    const int r0 = ((int)blockIdx.x / tiles_x) * kSsimTH, c0 = ((int)blockIdx.x % tiles_x) * kSsimTW;
    const int out_h = n_cells - w + 1, out_w = n_angles - w + 1;

    // positions past the last window read zeros; they are masked below
    for (int e = threadIdx.x; e < in_h * in_w; e += kSsimTB) {
        const int r = r0 + e / in_w, c = c0 + e % in_w;
        const bool in = r < n_cells && c < n_angles;
        const size_t at = (size_t)(in ? r : 0) * n_angles + (in ? c : 0);
        const uint8_t x = img[at], y = ref[at];
        tx[e] = in ? x : (uint8_t)0; ty[e] = in ? y : (uint8_t)0;
    }
    __syncthreads();
    // horizontal: w x 255 fits 16 bits, w x 255^2 fits 20
    for (int e = threadIdx.x; e < in_h * kSsimTW; e += kSsimTB) {
        const int r = e / kSsimTW, j = e % kSsimTW;
        const uint8_t* px = tx + r * in_w + j; const uint8_t* py = ty + r * in_w + j;
        uint32_t sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
        for (int k = 0; k < w; k++) {
            const uint32_t x = px[k], y = py[k];
            sx += x; sy += y; sxx += x * x; syy += y * y; sxy += x * y;
        }
        hs[e] = make_uint4(sx | (sy << 16), sxx, syy, sxy);
    }
    __syncthreads();
    // vertical: w^2 x 255 = 57,375 at w = 15 still fits the 16-bit halves, w^2 x 255^2 fits 32 bits
    const int j = threadIdx.x % kSsimTW, i0 = (threadIdx.x / kSsimTW) * kSsimRows;
    uint4 acc = make_uint4(0, 0, 0, 0);
    for (int k = 0; k < w; k++) {
        const uint4 v = hs[(i0 + k) * kSsimTW + j];
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    const double np = (double)(w * w), inv_np = 1.0 / np, cov_norm = np / (np - 1.0);
    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    double local = 0.0;
    for (int i = i0; i < i0 + kSsimRows; i++) {
        const double ux = (double)(acc.x & 0xFFFFu) * inv_np, uy = (double)(acc.x >> 16) * inv_np;
        const double uxx = (double)acc.y * inv_np, uyy = (double)acc.z * inv_np, uxy = (double)acc.w * inv_np;
        const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
        const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2;
        const double B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
        const double S = (A1 * A2) / (B1 * B2);
        local += (r0 + i < out_h && c0 + j < out_w) ? S : 0.0;
        if (i + 1 < i0 + kSsimRows) {
            const uint4 in = hs[(i + w) * kSsimTW + j], out = hs[i * kSsimTW + j];
            acc.x += in.x - out.x; acc.y += in.y - out.y; acc.z += in.z - out.z; acc.w += in.w - out.w;
        }
    }
    const double total = block_sum(local, s_part);
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// grid n_images, block 256.  hist / ssim_part / sse: null when that metric was not asked for (its fields stay 0; psnr is the
// host's to fill from sse, with the expression rr_score_images_device uses)
__global__ void __launch_bounds__(256) k_metrics_finish(const uint32_t* __restrict__ hist, const double* __restrict__ ssim_part, int n_blocks,
                                                        double ssim_count, const unsigned long long* __restrict__ sse, double n_px,
                                                        rr_image_metrics* out)
{
    __shared__ uint32_t row[256];
    __shared__ double s_part[4];
    const int t = threadIdx.x, img = blockIdx.x;
    rr_image_metrics m;
    m.psnr = 0.0; m.sse = sse ? sse[img] : 0ull;
    m.ssim = m.hx = m.hy = m.hxy = m.mi = m.nmi = m.voi = 0.0;
    if (hist) {
        const uint32_t* H = hist + (size_t)img * 65536;
        row[t] = 0;
        __syncthreads();
        // c (ln N - ln c) summed instead of ln N - (1/N) sum c ln c: the same number, and exactly 0 for a bin that holds all N
        const double ln_n = log(n_px);
        uint32_t col = 0;
        double sxy = 0.0;
        for (int r = 0; r < 256; r++) {
            const uint32_t c = H[r * 256 + t];
            col += c;
            if (c) sxy += (double)c * (ln_n - log((double)c));
            uint32_t rs = c;
            for (int off = 32; off > 0; off >>= 1) rs += __shfl_down(rs, off);
            if ((t & 63) == 0 && rs) atomicAdd(&row[r], rs);
        }
        __syncthreads();
        const uint32_t rx = row[t];
        const double sx = rx ? (double)rx * (ln_n - log((double)rx)) : 0.0;
        const double sy = col ? (double)col * (ln_n - log((double)col)) : 0.0;
        m.hxy = block_sum(sxy, s_part) / n_px;
        m.hx = block_sum(sx, s_part) / n_px;
        m.hy = block_sum(sy, s_part) / n_px;
        m.mi = m.hx + m.hy - m.hxy;
        m.nmi = m.hxy == 0.0 ? 1.0 : (m.hx + m.hy) / m.hxy;
        m.voi = 2.0 * m.hxy - m.hx - m.hy;
    }
    if (ssim_part) {
        const double* p = ssim_part + (size_t)img * n_blocks;
        double s = 0.0;
        for (int b = t; b < n_blocks; b += 256) s += p[b];
        m.ssim = block_sum(s, s_part) / ssim_count;
    }
    if (t == 0) out[img] = m;
}

}  // namespace

void launch_joint_hist(const uint8_t* imgs, const uint8_t* ref, size_t npx, int n_images, uint32_t* hist, int shape, hipStream_t s)
{
    const dim3 grid((unsigned)((npx + kHistStrip - 1) / kHistStrip), (unsigned)n_images);
    if (shape == 0) hipLaunchKernelGGL(k_joint_hist<true>, grid, dim3(kHistTB), 0, s, imgs, ref, npx, hist);
    else hipLaunchKernelGGL(k_joint_hist<false>, grid, dim3(256), 0, s, imgs, ref, npx, hist);
}

int ssim_blocks(int n_cells, int n_angles, int win)
{
    return ((n_cells - win + 1 + kSsimTH - 1) / kSsimTH) * ((n_angles - win + 1 + kSsimTW - 1) / kSsimTW);
}

void launch_ssim(const uint8_t* imgs, const uint8_t* ref, int n_cells, int n_angles, int win, int n_images, double* partial, hipStream_t s)
{
    const int tiles_x = (n_angles - win + 1 + kSsimTW - 1) / kSsimTW;
    hipLaunchKernelGGL(k_ssim, dim3((unsigned)ssim_blocks(n_cells, n_angles, win), (unsigned)n_images), dim3(kSsimTB), ssim_lds(win), s,
                       imgs, ref, n_cells, n_angles, win, tiles_x, partial);
}

void launch_metrics_finish(const uint32_t* hist, const double* ssim_part, int n_blocks, double ssim_count, const unsigned long long* sse,
                           size_t npx, rr_image_metrics* out, int n_images, hipStream_t s)
{
    hipLaunchKernelGGL(k_metrics_finish, dim3((unsigned)n_images), dim3(256), 0, s, hist, ssim_part, n_blocks, ssim_count, sse, (double)npx, out);
}

}  // namespace rr
