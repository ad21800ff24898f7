// rr_slice.hip -- gfx950 kernels of mesh maps (rr_slice_mesh_device; the definition is in include/radarays_mi355.h): the context's posed
// triangles sliced into the grid map of rr_field_config.  Every cell whose closed column [ix, ix+1] x [iy, iy+1] x [z_lo, z_hi] some
// triangle touches gets a byte 1, and with an object plane the smallest object id among those triangles.
//
//   k_slice_small   one thread per triangle record, kSliceTB per workgroup.  Face and object of the record, the skip byte, the posed corners
//                   (posed_face, rr_posed.h), then the z reject on the raw values -- it removes nearly all of a city mesh, so it comes
//                   before the first division.  The survivors go into cell space (cell_coord, rr_grid.h) and get their candidate box; a box
//                   of at most kSliceSmallCells cells is tested cell by cell in the thread, any other record's index is appended to the
//                   large list in scratch (one atomicAdd on the counter in front of it; the list's order does not reach the result)
//   k_slice_large   kSliceLargeGroups workgroups, launched always, the list's length read on the device.  A workgroup takes list entries
//                   grid-stride; every lane forms the entry's triangle again (the same addresses in every lane: one fetch per wave), so
//                   nothing is handed over through LDS and there is no barrier.  A wave takes the candidate box's kSliceTile x kSliceTile
//                   tiles 64 at a time, one tile per lane, through the prefilter: the same separating-axis test against the tile grown by a
//                   whole cell (and its band by 2^-16), which cannot drop a cell the predicate marks.  The tiles that pass
//                   are taken in turn (a ballot, wave-uniform), one cell per lane
//
// The predicate (slice_overlap) is the header's, operation by operation; tests/slice_ref.py restates it.  Every store of a byte is the
// same 1 whoever writes it, the object plane takes atomicMin: neither the order nor the number of writers reaches the result, so the
// several records of a face that spatial splits cut are harmless.  Every scalar travels as a kernel argument.  No scratch memory (private),
// no LDS, no barrier in either kernel; plain vector stores and vector atomics only.
#include "../../include/radarays_mi355.h"
#include "rr_bvh.h"
#include "rr_device.h"
#include "rr_grid.h"
#include "rr_launch.h"
#include "rr_posed.h"

namespace rr {

namespace {

constexpr int kSliceTB = 256;                 // threads of a workgroup of either kernel: four waves
constexpr int kSliceSmallCells = 64;          // a candidate box of at most this many cells is tested in its record's thread
constexpr int kSliceTile = 8;                 // side of a tile of k_slice_large: 64 cells, one per lane
constexpr int kSliceLargeGroups = 256;        // workgroups of k_slice_large: one per CU
constexpr float kSliceTileHalf = 0.5f * kSliceTile + 1.0f;      // half side of a tile grown by a whole cell
constexpr float kSliceBandGrow = 1.0f + 0x1p-16f;               // ... and what the prefilter grows the band's half height by

static_assert(sizeof(rr_field_config) == 32 && sizeof(rr_slice_config) == 16, "the grid is 32 bytes, the band 16");
static_assert(kSliceTile * kSliceTile == 64 && kSliceTB % 64 == 0, "a tile is one cell per lane");

// a triangle in (u, v, z): corners, edges e_j = corner (j+1) - corner j formed from the raw corners, the normal e0 x e1
struct SliceTri {
    float u0, u1, u2, v0, v1, v2, z0, z1, z2;
    float e0u, e0v, e0z, e1u, e1v, e1z, e2u, e2v, e2z;
    float nu, nv, nz;
};
// ... and its candidate box, clamped to the grid in float before the conversion
struct SliceBox { int xlo, xhi, ylo, yhi; };

// both projections strictly beyond the radius on the same side (false for a NaN: a reject needs an inequality that holds)
__device__ inline bool apart2(float a, float b, float r) { return (a > r && b > r) || (a < -r && b < -r); }

// the three cross-product axes of one edge (eu, ev, ez) against corners a and b, centred: (1,0,0) x e, (0,1,0) x e, (0,0,1) x e
__device__ inline bool edge_apart(float eu, float ev, float ez, float au, float av, float az, float bu, float bv, float bz, float hu, float hv, float hz)
{
    if (apart2(ez * av - ev * az, ez * bv - ev * bz, hv * fabsf(ez) + hz * fabsf(ev))) return true;
    if (apart2(eu * az - ez * au, eu * bz - ez * bu, hu * fabsf(ez) + hz * fabsf(eu))) return true;
    return apart2(ev * au - eu * av, ev * bu - eu * bv, hu * fabsf(ev) + hv * fabsf(eu));
}

// no separating axis among the normal and the nine edge axes between T and the box of centre (cu, cv, cz) and half sides (hu, hv, hz); the
// three box axes are the caller's (the candidate box, the z reject).  The corners are centred on the box first, then the products are formed
__device__ inline bool slice_overlap(const SliceTri& T, float cu, float cv, float cz, float hu, float hv, float hz)
{
    const float pu0 = T.u0 - cu, pu1 = T.u1 - cu, pu2 = T.u2 - cu;
    const float pv0 = T.v0 - cv, pv1 = T.v1 - cv, pv2 = T.v2 - cv;
    const float pz0 = T.z0 - cz, pz1 = T.z1 - cz, pz2 = T.z2 - cz;
    const float d = (T.nu * pu0 + T.nv * pv0) + T.nz * pz0;
    const float r = (hu * fabsf(T.nu) + hv * fabsf(T.nv)) + hz * fabsf(T.nz);
    if (d > r || d < -r) return false;
    if (edge_apart(T.e0u, T.e0v, T.e0z, pu0, pv0, pz0, pu2, pv2, pz2, hu, hv, hz)) return false;      // edge j against corners j and j + 2
    if (edge_apart(T.e1u, T.e1v, T.e1z, pu1, pv1, pz1, pu0, pv0, pz0, hu, hv, hz)) return false;
    if (edge_apart(T.e2u, T.e2v, T.e2z, pu2, pv2, pz2, pu1, pv1, pz1, hu, hv, hz)) return false;
    return true;
}

// record i -> its triangle, object and candidate box; false: skipped, rejected, not finite or outside the grid
__device__ inline bool slice_record(const TriRec* __restrict__ tris, size_t i, const float* __restrict__ verts, const uint32_t* __restrict__ faces,
                                    const float* __restrict__ poses, const uint8_t* __restrict__ skip, float z_lo, float z_hi,
                                    const rr_field_config& g, SliceTri& T, SliceBox& B, uint32_t& object)
{
    const uint32_t face = tris[i].face;
    object = tris[i].object;
    if (skip && skip[object]) return false;
    V3 a, b, c;
    posed_face(verts, faces, poses, face, object, a, b, c);
    // the band, on the raw values; a NaN rejects nothing here and is caught below
    if ((a.z < z_lo && b.z < z_lo && c.z < z_lo) || (a.z > z_hi && b.z > z_hi && c.z > z_hi)) return false;
    T.u0 = cell_coord(a.x, g.x0, g.cell); T.u1 = cell_coord(b.x, g.x0, g.cell); T.u2 = cell_coord(c.x, g.x0, g.cell);
    T.v0 = cell_coord(a.y, g.y0, g.cell); T.v1 = cell_coord(b.y, g.y0, g.cell); T.v2 = cell_coord(c.y, g.y0, g.cell);
    T.z0 = a.z; T.z1 = b.z; T.z2 = c.z;
    if (!(isfinite(T.u0) && isfinite(T.u1) && isfinite(T.u2) && isfinite(T.v0) && isfinite(T.v1) && isfinite(T.v2) && isfinite(T.z0) && isfinite(T.z1) &&
          isfinite(T.z2)))
        return false;
    // cells whose closed interval [ix, ix + 1] meets [min u, max u]: ceil(min u) - 1 .. floor(max u), clamped in float
    const float xlo = fmaxf(ceilf(fminf(fminf(T.u0, T.u1), T.u2)) - 1.0f, 0.0f);
    const float xhi = fminf(floorf(fmaxf(fmaxf(T.u0, T.u1), T.u2)), (float)(g.width - 1));
    const float ylo = fmaxf(ceilf(fminf(fminf(T.v0, T.v1), T.v2)) - 1.0f, 0.0f);
    const float yhi = fminf(floorf(fmaxf(fmaxf(T.v0, T.v1), T.v2)), (float)(g.height - 1));
    if (!(xlo <= xhi && ylo <= yhi)) return false;
    B.xlo = (int)xlo; B.xhi = (int)xhi; B.ylo = (int)ylo; B.yhi = (int)yhi;
    T.e0u = T.u1 - T.u0; T.e0v = T.v1 - T.v0; T.e0z = T.z1 - T.z0;
    T.e1u = T.u2 - T.u1; T.e1v = T.v2 - T.v1; T.e1z = T.z2 - T.z1;
    T.e2u = T.u0 - T.u2; T.e2v = T.v0 - T.v2; T.e2z = T.z0 - T.z2;
    T.nu = T.e0v * T.e1z - T.e0z * T.e1v;
    T.nv = T.e0z * T.e1u - T.e0u * T.e1z;
    T.nz = T.e0u * T.e1v - T.e0v * T.e1u;
    return true;
}

// cell (ix, iy) of the grid, inside the candidate box: the predicate, and the stores of a marked cell
__device__ inline void slice_cell(const SliceTri& T, int ix, int iy, float cz, float hz, int width, uint32_t object, uint8_t* __restrict__ occ,
                                  uint32_t* __restrict__ objects)
{
    if (!slice_overlap(T, (float)ix + 0.5f, (float)iy + 0.5f, cz, 0.5f, 0.5f, hz)) return;
    const size_t at = (size_t)iy * width + ix;
    occ[at] = 1;
    if (objects) atomicMin(objects + at, object);
}

__global__ void __launch_bounds__(kSliceTB) k_slice_small(const TriRec* __restrict__ tris, uint32_t n, const float* __restrict__ verts,
                                                          const uint32_t* __restrict__ faces, const float* __restrict__ poses,
                                                          const uint8_t* __restrict__ skip, float z_lo, float z_hi, float cz, float hz, rr_field_config g,
                                                          uint8_t* __restrict__ occ, uint32_t* __restrict__ objects, uint32_t* __restrict__ scratch)
{
    const uint32_t i = blockIdx.x * (uint32_t)kSliceTB + threadIdx.x;
    if (i >= n) return;
    SliceTri T; SliceBox B; uint32_t object;
    if (!slice_record(tris, i, verts, faces, poses, skip, z_lo, z_hi, g, T, B, object)) return;
    if ((B.xhi - B.xlo + 1) * (B.yhi - B.ylo + 1) > kSliceSmallCells) {          // (at most 4096 x 4096)
        scratch[1 + atomicAdd(scratch, 1u)] = i;
        return;
    }
    for (int iy = B.ylo; iy <= B.yhi; iy++)
        for (int ix = B.xlo; ix <= B.xhi; ix++) slice_cell(T, ix, iy, cz, hz, g.width, object, occ, objects);
}

__global__ void __launch_bounds__(kSliceTB) k_slice_large(const TriRec* __restrict__ tris, uint32_t n, const float* __restrict__ verts,
                                                          const uint32_t* __restrict__ faces, const float* __restrict__ poses, float z_lo, float z_hi,
                                                          float cz, float hz, rr_field_config g, uint8_t* __restrict__ occ,
                                                          uint32_t* __restrict__ objects, const uint32_t* __restrict__ scratch)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t count = min(scratch[0], n);
    const float hz_tile = hz * kSliceBandGrow;
    for (uint32_t e = blockIdx.x; e < count; e += gridDim.x) {
        SliceTri T; SliceBox B; uint32_t object;
        if (!slice_record(tris, scratch[1 + e], verts, faces, poses, nullptr, z_lo, z_hi, g, T, B, object)) continue;     // (it passed once: the same values)
        const int ntx = (B.xhi - B.xlo + kSliceTile) / kSliceTile, nty = (B.yhi - B.ylo + kSliceTile) / kSliceTile;
        const int n_tiles = ntx * nty;                                        // (at most 512 x 512)
        for (int t0 = wave * 64; t0 < n_tiles; t0 += (kSliceTB / 64) * 64) {
            const int t = t0 + lane;
            bool pass = false;
            if (t < n_tiles) {
                const int ty = t / ntx, tx = t - ty * ntx;
                pass = slice_overlap(T, (float)(B.xlo + kSliceTile * tx) + 0.5f * kSliceTile, (float)(B.ylo + kSliceTile * ty) + 0.5f * kSliceTile, cz,
                                     kSliceTileHalf, kSliceTileHalf, hz_tile);
            }
            unsigned long long todo = __ballot(pass);
            while (todo) {
                const int tt = t0 + (__ffsll((long long)todo) - 1);
                todo &= todo - 1;
                const int ty = tt / ntx, tx = tt - ty * ntx;
                const int ix = B.xlo + kSliceTile * tx + (lane & (kSliceTile - 1)), iy = B.ylo + kSliceTile * ty + lane / kSliceTile;
                if (ix <= B.xhi && iy <= B.yhi) slice_cell(T, ix, iy, cz, hz, g.width, object, occ, objects);
            }
        }
    }
}

}  // namespace

void slice_tile_sizes(int* small_cells, int* tile_side, int* group_size)
{
    if (small_cells) *small_cells = kSliceSmallCells;
    if (tile_side) *tile_side = kSliceTile;
    if (group_size) *group_size = kSliceTB;
}

int slice_large_groups() { return kSliceLargeGroups; }

size_t slice_scratch_words(size_t n_records) { return n_records + 1; }

void launch_slice(const TriRec* tris, size_t n, const float* verts, const uint32_t* faces, const float* poses, const uint8_t* skip,
                  const rr_slice_config& sc, const rr_field_config& g, uint8_t* occ, uint32_t* objects, uint32_t* scratch, hipStream_t s)
{
    if (n == 0) return;
    // the band's centre and half height, one f32 operation each after the sum and the difference
    const float cz = (sc.z_lo + sc.z_hi) * 0.5f, hz = (sc.z_hi - sc.z_lo) * 0.5f;
    (void)hipMemsetAsync(scratch, 0, sizeof(uint32_t), s);
    hipLaunchKernelGGL(k_slice_small, dim3((unsigned)((n + kSliceTB - 1) / kSliceTB)), dim3(kSliceTB), 0, s, tris, (uint32_t)n, verts, faces, poses, skip,
                       sc.z_lo, sc.z_hi, cz, hz, g, occ, objects, scratch);
    hipLaunchKernelGGL(k_slice_large, dim3(kSliceLargeGroups), dim3(kSliceTB), 0, s, tris, (uint32_t)n, verts, faces, poses, sc.z_lo, sc.z_hi, cz, hz, g,
                       occ, objects, scratch);
}

}  // namespace rr
