// rr_polar.h -- the geometry of a polar image [n_cells][n_angles], stated once for the detectors, the annotations and the three Cartesian
// resamplers (rr_detect.hip, rr_notes.hip, rr_deskew.hip) and for the scan profiles of the map kernels (rr_occupancy.hip, rr_cast.hip).  Image column col holds azimuth index a = col - scroll (mod n_angles), which
// lies a steps of theta_inc from theta_min; range bin b lies at (b + 0.5) * resolution.  A point at yaw phi and range rho has the continuous
// coordinates u = (phi - theta_min) / theta_inc (mod n_angles) and v = rho / res - 0.5.  All f32 but the bin's range, nothing fused.
#pragma once
#include "../../include/radarays_mi355.h"
#include "rr_device.h"

namespace rr {

struct PolarGrid {
    int n_cells, n_angles, scroll;      // scroll in [0, n_angles)
    float theta_min, theta_inc;
    float res;                          // (float)resolution: the resamplers divide by it
    double resolution;                  // the detectors, the annotations and the compensated points multiply by it
};

inline PolarGrid polar_grid(const rr_config& c)
{
    const int n_angles = c.n_angles, scroll = ((c.scroll_image % n_angles) + n_angles) % n_angles;
    return { c.n_cells, n_angles, scroll, c.theta_min, c.theta_inc, (float)c.resolution, c.resolution };
}

struct CartGrid { int width; float pixel_size; };       // a square Cartesian image, the sensor at its centre

__device__ inline int az_of_col(const PolarGrid& G, int col) { return col - G.scroll < 0 ? col - G.scroll + G.n_angles : col - G.scroll; }
__device__ inline int col_of_az(const PolarGrid& G, int a)
{
    int col = a + G.scroll;
    if (col >= G.n_angles) col -= G.n_angles;
    return col;
}
__device__ inline float az_theta(const PolarGrid& G, int a) { return G.theta_min + (float)a * G.theta_inc; }
template <class I> __device__ inline float bin_range(const PolarGrid& G, I b) { return (float)(((double)b + 0.5) * G.resolution); }

// the first detection of image column col of one frame's point list (the points of a column are sorted by bin; offs: the frame's n_angles + 1
// offsets): true and its bin.  False where the column has no detection, and with *cut where every detection of it lies past max_points
__device__ inline bool column_first_bin(const rr_radar_point* frame_points, const uint32_t* offs, int col, int max_points, uint32_t* bin, bool* cut)
{
    const uint32_t first = offs[col], next = offs[col + 1];
    *cut = next > first && first >= (uint32_t)max_points;
    if (next <= first || *cut) return false;
    *bin = frame_points[first].bin;
    return true;
}

// the azimuth coordinate of a yaw, always in [0, n_angles)
__device__ inline float az_coord(const PolarGrid& G, float phi)
{
    const float na = (float)G.n_angles;
    float u = fmodf((phi - G.theta_min) / G.theta_inc, na);
    if (u < 0.0f) u += na;
    if (u >= na) u -= na;
    if (!(u >= 0.0f && u < na)) u = 0.0f;      // (a non-finite yaw, or a theta_inc so small that the quotient overflows)
    return u;
}
__device__ inline int az_nearest(const PolarGrid& G, float u)
{
    int a = (int)rintf(u);
    if (a >= G.n_angles) a -= G.n_angles;
    return a;
}
// the range coordinate of a range, clamped at bin 0; false beyond the last bin (what a pixel holds there is the caller's)
__device__ inline bool range_coord(const PolarGrid& G, float rho, float* v)
{
    const float x = rho / G.res - 0.5f;
    if (!(x <= (float)G.n_cells - 0.5f)) return false;
    *v = fmaxf(x, 0.0f);
    return true;
}

// bin b of azimuth a: uint8 images and uint32 label planes alike
template <class T> __device__ inline T polar_at(const T* img, const PolarGrid& G, int b, int a) { return img[(size_t)b * G.n_angles + col_of_az(G, a)]; }

template <class T> __device__ inline T polar_nearest(const T* img, const PolarGrid& G, float u, float v)
{
    const int a = az_nearest(G, u);
    return polar_at(img, G, min((int)rintf(v), G.n_cells - 1), a);
}
__device__ inline uint8_t polar_bilinear(const uint8_t* img, const PolarGrid& G, float u, float v)
{
    const int a0 = min((int)floorf(u), G.n_angles - 1);
    const int a1 = a0 + 1 == G.n_angles ? 0 : a0 + 1;
    const float fu = u - (float)a0;
    const int b0 = (int)floorf(v), b1 = min(b0 + 1, G.n_cells - 1);
    const float fv = v - (float)b0;
    const int z00 = polar_at(img, G, b0, a0), z01 = polar_at(img, G, b0, a1), z10 = polar_at(img, G, b1, a0), z11 = polar_at(img, G, b1, a1);
    const float p0 = (1.0f - fu) * (float)z00 + fu * (float)z01;
    const float p1 = (1.0f - fu) * (float)z10 + fu * (float)z11;
    const float val = rintf((1.0f - fv) * p0 + fv * p1);
    return (uint8_t)fminf(fmaxf(val, 0.0f), 255.0f);
}
// INTERP: 0 nearest, 1 bilinear
template <int INTERP> __device__ inline uint8_t polar_sample(const uint8_t* img, const PolarGrid& G, float u, float v)
{
    return INTERP == 0 ? polar_nearest(img, G, u, v) : polar_bilinear(img, G, u, v);
}

// the sensor-frame place of pixel (i, j): x forward is up, y left is left
template <class I> __device__ inline V3 pixel_xy(const CartGrid& C, I i, I j)
{
    const float cc = (float)(C.width - 1) * 0.5f;
    return { (cc - (float)i) * C.pixel_size, (cc - (float)j) * C.pixel_size, 0.0f };
}

}  // namespace rr
