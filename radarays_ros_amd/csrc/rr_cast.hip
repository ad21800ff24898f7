// rr_cast.hip -- gfx950 kernels of the beam model (rr_scan_profile_device, rr_cast_map_device, rr_score_beams_device; the definition is in
// include/radarays_mi355.h): a scan's first detection per azimuth, the grid map cast at pose hypotheses, and a scan's rays scored against it.
//
//   k_scan_profile    grid (azimuth tiles, frames), one thread per (frame, azimuth): the bin of the first detection of the azimuth's image
//                     column (the points of a column are sorted by bin), n_cells where there is none or it was cut by max_points
//   k_cast<SCORE>     the hot path, one body for both ray calls.  Lanes over azimuths: a wave owns whole hypotheses, kCastHypsPerWave of
//                     them in turn, whose state is wave-uniform, and walks n_angles kCastAnglesTile = 64 at a time.  Neighbouring azimuths
//                     walk neighbouring cells and have similar lengths, so a wave's 2-byte gathers fall into few lines and its lanes leave
//                     the march at similar step counts.  A lane marches ONE ray: at an IN GRID sample whose field value d2 is not 0 the
//                     samples that d2 proves empty are skipped (the rule and its proof: DESIGN.md §27; tests/cast_ref.py holds it to the
//                     march over every sample), outside the grid it steps by one.
//                     SCORE = false stores e[a] (rr_cast_map).  SCORE = true classifies e[a] against the scan's profile and keeps the six
//                     counts and sum_abs per lane; they are reduced across the wave with shuffles and lane 0 stores the record: a
//                     hypothesis never leaves its wave, so there are no atomics, no zeroing launch, no LDS and no barrier.  An azimuth the
//                     profile leaves out (m < bin_begin) is not cast at all
//
// Every scalar travels as a kernel argument.  No scratch memory and no LDS in any kernel of the file.
#include "../../include/radarays_mi355.h"
#include "rr_device.h"
#include "rr_grid.h"
#include "rr_launch.h"
#include "rr_polar.h"
#include "rr_pose2d.h"

namespace rr {

namespace {

constexpr int kCastTB = 256;                                     // threads of a k_cast workgroup: four waves
constexpr int kCastAnglesTile = 64;                              // azimuths a wave takes per step: one per lane
constexpr int kCastHypsPerWave = 4;                              // hypotheses a wave takes in turn
constexpr int kCastHypsPerGroup = (kCastTB / 64) * kCastHypsPerWave;    // 16

// the margins of the skip rule; tests/cast_ref.py restates them
constexpr float kCastEps = 0x1p-22f;                             // four unit roundoffs per unit of coordinate magnitude
constexpr float kCastSlack = 0x1p-8f;                            // cells: the roundings of u and v of two samples inside a grid of 4096
constexpr float kCastDiag = 1.5f;                                // cells: above sqrt(2), two half diagonals of a cell
constexpr float kCastTiny = 0x1p-120f;                           // above what two squares can lose to underflow
constexpr float kCastMaxSkip = 65536.0f;

static_assert(sizeof(rr_field_config) == 32 && sizeof(rr_beam_config) == 32 && sizeof(rr_beam_rec) == 32, "the grid, the beams and a record: 32 bytes");
static_assert(sizeof(rr_radar_point) == 24, "a 24-byte point");

__global__ void __launch_bounds__(256) k_scan_profile(const rr_radar_point* __restrict__ points, const uint32_t* __restrict__ offsets, int max_points,
                                                      PolarGrid G, uint16_t* __restrict__ first_bin)
{
    const int f = blockIdx.y, a = blockIdx.x * 256 + threadIdx.x;
    if (a >= G.n_angles) return;
    uint32_t fb = (uint32_t)G.n_cells, bin;
    bool cut;
    if (column_first_bin(points + (size_t)f * max_points, offsets + (size_t)f * (G.n_angles + 1), col_of_az(G, a), max_points, &bin, &cut))
        fb = min(bin, (uint32_t)G.n_cells);
    first_bin[(size_t)f * G.n_angles + a] = (uint16_t)fb;
}

// what a ray's march needs beside its direction; the same for every lane of a wave
struct CastWave {
    Pose2 p;                     // the hypothesis (c, s, tx, ty)
    float len_cs, m1, t1;        // sqrt(c*c + s*s + tiny), |c| + |s|, |tx| + |ty|
};

// e of one ray: the smallest sampled bin that is a hit, bin_end if there is none
__device__ inline int cast_ray(const CastWave& w, float ca, float sa, const uint16_t* __restrict__ field, const rr_field_config& g, int bin_begin,
                               int bin_end, int bin_step, double resolution, float step_m, float r_max, float shrink)
{
    // cells between two samples, from above, and its inverse from below; the rounding of two samples' cell coordinates, from above
    const float len_d = sqrtf((ca * ca + sa * sa) + kCastTiny);
    const float inv_g = shrink / (((step_m * len_d) * w.len_cs) / g.cell);
    const float big = (w.m1 * (fabsf(ca) + fabsf(sa))) * r_max;
    const float err = (kCastEps * (16.0f * big + w.t1)) / g.cell + kCastSlack;
    int b = bin_begin;
    while (b < bin_end) {
        const float r = (float)(((double)b + 0.5) * resolution);
        float px, py;
        pose_move(w.p, r * ca, r * sa, &px, &py);
        const GridCell q = grid_cell(px, py, g);
        int advance = 1;
        if (q.in) {
            const uint32_t d2 = field[grid_index(q, g)];
            if (d2 == 0) break;                                  // a hit: e = b
            const float q = ((floorf(sqrtf((float)d2)) - kCastDiag) - err) * inv_g;
            if (q >= 1.0f) advance += (int)fminf(q, kCastMaxSkip);      // (false for a NaN)
        }
        b += advance * bin_step;                                 // (at most 65,537 * 64 past bin_end)
    }
    return min(b, bin_end);
}

template <bool SCORE>
__global__ void __launch_bounds__(kCastTB) k_cast(const float* __restrict__ states, int n_hyp, const float* __restrict__ dirs, int n_angles,
                                                  const uint16_t* __restrict__ field, rr_field_config g, rr_beam_config bc, double resolution,
                                                  float step_m, float r_max, float shrink, const uint16_t* __restrict__ first_bin,
                                                  uint16_t* __restrict__ ranges, rr_beam_rec* __restrict__ recs)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int h0 = ((int)blockIdx.x * (kCastTB / 64) + wave) * kCastHypsPerWave;
    for (int t = 0; t < kCastHypsPerWave; t++) {
        const int h = h0 + t;
        if (h >= n_hyp) return;                                   // (the whole wave; the kernel has no barrier)
        CastWave w;
        w.p = pose_of(states, (size_t)h);
        w.len_cs = sqrtf((w.p.c * w.p.c + w.p.s * w.p.s) + kCastTiny);
        w.m1 = fabsf(w.p.c) + fabsf(w.p.s);
        w.t1 = fabsf(w.p.tx) + fabsf(w.p.ty);

        uint32_t n_agree = 0, n_short = 0, n_through = 0, n_open = 0, n_none = 0, n_cast = 0;
        unsigned long long sum_abs = 0;
        for (int a0 = 0; a0 < n_angles; a0 += kCastAnglesTile) {
            const int a = a0 + lane;
            if (a >= n_angles) continue;                          // (a0 is uniform: the lanes past the last azimuth sit this step out)
            int m = 0;
            if (SCORE) {
                m = first_bin[a];
                if (m < bc.bin_begin) continue;                   // left out, and not cast
            }
            const int e = cast_ray(w, dirs[2 * (size_t)a], dirs[2 * (size_t)a + 1], field, g, bc.bin_begin, bc.bin_end, bc.bin_step, resolution,
                                   step_m, r_max, shrink);
            if (!SCORE) {
                ranges[(size_t)h * n_angles + a] = (uint16_t)e;
                continue;
            }
            const bool e_none = e >= bc.bin_end, m_none = m >= bc.bin_end;
            n_cast++;
            if (e_none) { n_none += m_none ? 1u : 0u; n_open += m_none ? 0u : 1u; }
            else if (m_none) n_through++;
            else {
                const int d = m - e, ad = d < 0 ? -d : d;
                n_agree += ad <= bc.tol_bins ? 1u : 0u;
                n_short += d < -bc.tol_bins ? 1u : 0u;
                n_through += d > bc.tol_bins ? 1u : 0u;
                sum_abs += (unsigned long long)min(ad, bc.clip_bins);
            }
        }
        if (!SCORE) continue;
        rr_beam_rec r;
        r.n_agree = wave_sum(n_agree); r.n_short = wave_sum(n_short); r.n_through = wave_sum(n_through);
        r.n_open = wave_sum(n_open); r.n_none = wave_sum(n_none); r.n_cast = wave_sum(n_cast);
        r.sum_abs = wave_sum(sum_abs);
        if (lane == 0) recs[h] = r;                               // plain vector stores, one record per hypothesis
    }
}

}  // namespace

void cast_tile_sizes(int* angles_tile, int* hyps_per_wave, int* hyps_per_group)
{
    if (angles_tile) *angles_tile = kCastAnglesTile;
    if (hyps_per_wave) *hyps_per_wave = kCastHypsPerWave;
    if (hyps_per_group) *hyps_per_group = kCastHypsPerGroup;
}

void launch_scan_profile(const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points, const PolarGrid& G, uint16_t* first_bin,
                         hipStream_t s)
{
    hipLaunchKernelGGL(k_scan_profile, dim3((unsigned)((G.n_angles + 255) / 256), (unsigned)n_frames), dim3(256), 0, s, points, offsets, max_points, G,
                       first_bin);
}

void launch_cast(const uint16_t* first_bin, const float* states, int n_hyp, const float* dirs, int n_angles, double resolution, const uint16_t* field,
                 const rr_field_config& g, const rr_beam_config& bc, uint16_t* ranges, rr_beam_rec* recs, hipStream_t s)
{
    const float step_m = fabsf((float)((double)bc.bin_step * resolution));
    const float r_max = fabsf((float)(((double)bc.bin_end + 0.5) * resolution));
    const float shrink = g.cell >= 0x1p-64f ? 1.0f - 0x1p-10f : 0.0f;      // (below that the underflow of a coordinate is not covered: no skip)
    const unsigned groups = (unsigned)((n_hyp + kCastHypsPerGroup - 1) / kCastHypsPerGroup);
    if (recs)
        hipLaunchKernelGGL(k_cast<true>, dim3(groups), dim3(kCastTB), 0, s, states, n_hyp, dirs, n_angles, field, g, bc, resolution, step_m, r_max,
                           shrink, first_bin, ranges, recs);
    else
        hipLaunchKernelGGL(k_cast<false>, dim3(groups), dim3(kCastTB), 0, s, states, n_hyp, dirs, n_angles, field, g, bc, resolution, step_m, r_max,
                           shrink, first_bin, ranges, recs);
}

}  // namespace rr
