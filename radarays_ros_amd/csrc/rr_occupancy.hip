// rr_occupancy.hip -- gfx950 kernels of occupancy mapping (rr_occupancy_update_device, rr_occupancy_map_device; the definition is in
// include/radarays_mi355.h): posed scans fused into an int32 evidence grid.  A detection adds l_hit to its cell, every cell a scan saw
// to be empty loses l_free, and the map call clamps the sums into a byte.
//
//   k_occ_profile     grid (column tiles, scans), one thread per (scan, column): where the azimuth's free space ends.  The first detection
//                     of the column (the points of a column are sorted by bin), moved in by margin_bins and cut at max_free_bin, as a
//                     squared range into free2[scan][azimuth]
//   k_occ_free        the hot path: cells x scans of the inverse sensor model.  A thread owns kOccCellsPerThread consecutive cells for the
//                     whole call and walks ALL scans: per scan the cell centres are moved into the sensor frame, atan2f gives the
//                     azimuth, and one gather from free2 answers "did this scan see the cell empty".  The count stays in a register; one
//                     plain read-modify-write per cell ends the kernel: no atomics, no LDS, no barrier.  The scan's state is wave-uniform
//                     (scalar loads); the kOccCellsPerThread atan2f chains are independent and in flight together.
//                     free2 is gathered from L1 / L2, not staged in LDS: by count the kernel is VALU-bound about eight to one over
//                     the gather, the cells of a wave are neighbours in a row and look at a narrow fan of azimuths, so
//                     a wave's gather falls into few cache lines of a row of 4 * n_angles bytes that stays in L1; and without a staged
//                     chunk there is no barrier, no limit on n_angles and no chunk edge
//   k_occ_hit         grid (point tiles, scans), one thread per point: the state's move and the cell rule (rr_pose2d.h, rr_grid.h), then one integer atomicAdd
//                     of l_hit.  Launched behind k_occ_free on the same stream: the read-modify-write there is not atomic
//   k_occ_map         one thread per cell: clamp(128 + evidence, 0, 255)
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

constexpr int kOccTB = 256;                                      // threads of a k_occ_free workgroup: four waves
constexpr int kOccCellsPerThread = 4;                            // consecutive cells a thread owns: four atan2f chains in flight
constexpr int kOccCellsPerGroup = kOccTB * kOccCellsPerThread;   // 1024

static_assert(sizeof(rr_field_config) == 32 && sizeof(rr_occupancy_config) == 32, "the grid and the model are 32 bytes each");
static_assert(sizeof(rr_radar_point) == 24, "x and y lead a 24-byte point");

__global__ void __launch_bounds__(256) k_occ_profile(const rr_radar_point* __restrict__ points, const uint32_t* __restrict__ offsets, int max_points,
                                                     PolarGrid G, int margin_bins, int max_free_bin, float* __restrict__ free2)
{
    const int f = blockIdx.y, col = blockIdx.x * 256 + threadIdx.x;
    if (col >= G.n_angles) return;
    long long fb = G.n_cells;                                    // no detection: free as far as max_free_bin allows
    uint32_t bin;
    bool cut;                                                    // every detection of the column lies past max_points: nothing is asserted
    if (column_first_bin(points + (size_t)f * max_points, offsets + (size_t)f * (G.n_angles + 1), col, max_points, &bin, &cut)) fb = bin;
    const long long free_bins = cut ? 0 : min(max(fb - margin_bins, 0ll), (long long)max_free_bin);
    const float r = (float)((double)free_bins * G.resolution);
    free2[(size_t)f * G.n_angles + az_of_col(G, col)] = r * r;
}

// the hot path.  cells = width * height; evidence is 4-byte aligned, `vec`: 16-byte aligned
__global__ void __launch_bounds__(kOccTB) k_occ_free(const float* __restrict__ free2, const double* __restrict__ states, int n_frames,
                                                     rr_field_config g, PolarGrid G, int l_free, int vec, int32_t* __restrict__ evidence)
{
    const uint32_t cells = (uint32_t)g.width * (uint32_t)g.height;
    const uint32_t q0 = ((uint32_t)blockIdx.x * kOccTB + threadIdx.x) * kOccCellsPerThread;
    if (q0 >= cells) return;
    float qx[kOccCellsPerThread], qy[kOccCellsPerThread];
    int n_free[kOccCellsPerThread];
#pragma unroll
    for (int e = 0; e < kOccCellsPerThread; e++) {
        const uint32_t q = min(q0 + e, cells - 1);               // a slot past the last cell repeats it and is not stored
        const uint32_t iy = q / (uint32_t)g.width, ix = q - iy * (uint32_t)g.width;
        qx[e] = cell_centre(g.x0, g.cell, ix);
        qy[e] = cell_centre(g.y0, g.cell, iy);
        n_free[e] = 0;
    }
    for (int f = 0; f < n_frames; f++) {
        const Pose2 st = pose_of(states, (size_t)f);             // wave-uniform
        const float* prof = free2 + (size_t)f * G.n_angles;
        int a[kOccCellsPerThread];
        float rho2[kOccCellsPerThread];
#pragma unroll
        for (int e = 0; e < kOccCellsPerThread; e++) {
            float px, py;
            pose_unmove(st, qx[e], qy[e], &px, &py);
            a[e] = az_nearest(G, az_coord(G, atan2f(py, px)));   // always inside [0, n_angles), whatever px and py are
            rho2[e] = px * px + py * py;
        }
        float lim[kOccCellsPerThread];
#pragma unroll
        for (int e = 0; e < kOccCellsPerThread; e++) lim[e] = prof[a[e]];         // kOccCellsPerThread independent gathers in flight
#pragma unroll
        for (int e = 0; e < kOccCellsPerThread; e++) n_free[e] += rho2[e] < lim[e] ? 1 : 0;   // a NaN or an infinite rho2 is never free
    }
    if (vec && q0 + kOccCellsPerThread <= cells) {
        int4* p = reinterpret_cast<int4*>(evidence + q0);
        int4 v = *p;
        v.x -= l_free * n_free[0]; v.y -= l_free * n_free[1]; v.z -= l_free * n_free[2]; v.w -= l_free * n_free[3];
        *p = v;
    } else {
#pragma unroll
        for (int e = 0; e < kOccCellsPerThread; e++)
            if (q0 + e < cells) evidence[q0 + e] -= l_free * n_free[e];
    }
}

__global__ void __launch_bounds__(256) k_occ_hit(const rr_radar_point* __restrict__ points, const uint32_t* __restrict__ offsets, int n_angles,
                                                 int max_points, const double* __restrict__ states, rr_field_config g, int l_hit, int32_t* evidence)
{
    const int f = blockIdx.y;
    const uint32_t m = frame_count(offsets, f, n_angles, max_points, nullptr);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    const Pose2 st = pose_of(states, (size_t)f);
    const rr_radar_point* src = points + (size_t)f * max_points;
    float px, py;
    pose_move(st, src[i].x, src[i].y, &px, &py);
    const GridCell q = grid_cell(px, py, g);
    if (q.in) atomicAdd(evidence + grid_index(q, g), l_hit);
}

__global__ void __launch_bounds__(256) k_occ_map(const int32_t* __restrict__ evidence, uint32_t cells, uint8_t* __restrict__ occ)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= cells) return;
    occ[q] = (uint8_t)(128 + min(max(evidence[q], -128), 127));  // clamp(128 + evidence, 0, 255) without the overflow
}

}  // namespace

void occupancy_tile_sizes(int* cells_per_group, int* cells_per_thread, int* scan_chunk)
{
    if (cells_per_group) *cells_per_group = kOccCellsPerGroup;
    if (cells_per_thread) *cells_per_thread = kOccCellsPerThread;
    if (scan_chunk) *scan_chunk = 0;                             // the profile is gathered, not staged: the scans are not chunked
}

void launch_occupancy_update(const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points, const double* states,
                             const rr_field_config& g, const rr_occupancy_config& o, const PolarGrid& G, float* profile, int32_t* evidence,
                             hipStream_t s)
{
    const unsigned cells = (unsigned)g.width * (unsigned)g.height;
    hipLaunchKernelGGL(k_occ_profile, dim3((unsigned)((G.n_angles + 255) / 256), (unsigned)n_frames), dim3(256), 0, s, points, offsets, max_points, G,
                       o.margin_bins, o.max_free_bin, profile);
    hipLaunchKernelGGL(k_occ_free, dim3((cells + kOccCellsPerGroup - 1) / kOccCellsPerGroup), dim3(kOccTB), 0, s, profile, states, n_frames, g, G,
                       o.l_free, (int)(reinterpret_cast<uintptr_t>(evidence) % 16 == 0), evidence);
    if (max_points <= 0) return;
    hipLaunchKernelGGL(k_occ_hit, dim3((unsigned)((max_points + 255) / 256), (unsigned)n_frames), dim3(256), 0, s, points, offsets, G.n_angles,
                       max_points, states, g, o.l_hit, evidence);
}

void launch_occupancy_map(const int32_t* evidence, const rr_field_config& g, uint8_t* occ, hipStream_t s)
{
    const unsigned cells = (unsigned)g.width * (unsigned)g.height;
    hipLaunchKernelGGL(k_occ_map, dim3((cells + 255) / 256), dim3(256), 0, s, evidence, cells, occ);
}

}  // namespace rr
