// rr_grid.h -- the grid map of rr_field_config, stated once for the likelihood field, occupancy mapping, map refinement and the beam model
// (rr_field.hip, rr_occupancy.hip, rr_refine.hip, rr_cast.hip) and for the mesh slicer (rr_slice.hip).  A map-frame point (px, py) has the cell coordinates u = (px - x0) / cell and
// v = (py - y0) / cell; it is IN GRID iff 0 <= u < width and 0 <= v < height, compared in float before any conversion to int, and then lies in
// cell (floor u, floor v), whose linear index is iy * width + ix and whose centre is x0 + (ix + 0.5) * cell.  All f32, nothing fused.
#pragma once
#include "../../include/radarays_mi355.h"
#include <hip/hip_runtime.h>

namespace rr {

constexpr int kGridMaxSide = 4096, kGridMaxDist = 255;           // width and height, max_dist: the calls refuse more, the row passes' LDS holds this much

// the cell rule of the header.  A NaN or an infinity fails the comparisons; a point that is not IN GRID gets cell (0, 0), an address that may be read
struct GridCell { bool in; int ix, iy; };
// the cell coordinate of a map-frame coordinate along one axis: origin is x0 or y0 (the mesh slicer takes a triangle's corners through it)
__device__ inline float cell_coord(float p, float origin, float cell) { return (p - origin) / cell; }
__device__ inline GridCell grid_cell(float px, float py, const rr_field_config& g)
{
    const float u = cell_coord(px, g.x0, g.cell), v = cell_coord(py, g.y0, g.cell);
    const bool in = u >= 0.0f && u < (float)g.width && v >= 0.0f && v < (float)g.height;
    return { in, in ? (int)floorf(u) : 0, in ? (int)floorf(v) : 0 };
}
__device__ inline uint32_t grid_index(const GridCell& q, const rr_field_config& g) { return (uint32_t)(q.iy * g.width + q.ix); }

// the centre of cell i along one axis: origin is x0 or y0
template <class I> __device__ inline float cell_centre(float origin, float cell, I i) { return origin + ((float)i + 0.5f) * cell; }

// one step of a column pass of either transform: the distance to the nearest occupied cell met so far, saturated at max_dist
__device__ inline int column_step(int d, bool occupied, int max_dist) { return occupied ? 0 : min(d + 1, max_dist); }

}  // namespace rr
