// rr_notes.hip -- gfx950 kernels that reduce label images to one record per object (rr_annotate_labels_device), attach the label under a
// detected point (rr_label_points_device) and resample uint32 planes to a Cartesian instance mask (rr_polar_to_cartesian_labels_device);
// the definitions are in include/radarays_mi355.h.
//
//   k_note_init          the identity of every accumulator record (16-B stores), the occupancy rows and the skip counts: nothing relies on a memset
//   k_note_accum         one workgroup per (tile of kNoteTW adjacent columns x chunk of kNoteRows range bins, frame).  A thread owns four
//                        adjacent columns (one 16-B load of labels, one 4-B load of the image per row) and walks down the chunk; the pixels
//                        of the object it is looking at are summed in registers and leave them only when the object changes.  They go to an
//                        LDS table keyed by object id (kNoteSlots entries, kNoteProbes linear probes, each entry the partial record and the
//                        tile's column-occupancy bits); at tile end every used entry is merged into the caller's scratch with integer
//                        global atomics.  A partial record that finds the table full goes straight to the same global atomics
//   k_note_finish        one group of kNoteGroup lanes per (frame, object): the largest circular gap of the occupancy row (a lane per word,
//                        a max-scan of the last occupied azimuth carries the gap across words), the packed peak key and the float keys
//                        unpacked, the record written as five 16-B stores
//   k_label_points       one thread per written point: the label, face and range rate under (bin, column)
//   k_cartesian_labels   one thread per output pixel: the nearest rule of rr_detect.hip's k_cartesian (rr_polar.h) on uint32
//
// Every reduction is over integers or a min / max (add, min, max, or; floats through the order-preserving integer mapping fkey), so a
// record does not depend on the order in which tiles and lanes arrive.
// Rests on: wave64 and 16-B per lane loads as the coalescing shape (cdna_hip_programming.md, Guidelines 2 and 13); partial reduction on
// chip before any global atomic (Guideline 12: registers, then LDS, one set of atomics per object and tile); LDS atomics are 32-lane-group
// operations with 32 banks for writes (MI355X_MICROARCH.md, LDS table), which the table's structure-of-arrays layout spreads by slot;
// atomics drop their line from the XCD's L2 (same file, store flavours), so the scratch is read back only by k_note_finish.
// Every value a call needs travels as a kernel argument; the kernels use no scratch memory and less than 8 KB of static LDS.
#include "../../include/radarays_mi355.h"
#include "rr_device.h"
#include "rr_launch.h"
#include "rr_polar.h"

#include <algorithm>

namespace rr {

namespace {

constexpr int kNoteTB = 256;            // threads of a k_note_accum workgroup: 8 column groups x 32 rows per sweep
constexpr int kNoteTW = 32;             // columns of a tile: one occupancy word
constexpr int kNoteRows = 256;          // range bins of a chunk: 8 sweeps, 32 pixels per thread behind its 8 trigonometric calls
constexpr int kNoteSlots = 128;         // entries of the LDS table
constexpr int kNoteProbes = 4;
constexpr int kNoteGroup = 16;          // lanes per (frame, object) of k_note_finish
constexpr uint32_t kNoId = 0xFFFFFFFFu; // no object: ids are below 2^24 - 1
constexpr int kAccWords = 16;           // a 64-byte accumulator record per (frame, object), words:
enum { A_ND = 0, A_NG, A_NM, A_NE, A_BMIN, A_BMAX, A_XMIN, A_XMAX, A_PEAK /* u64 */, A_SUM = 10 /* u64 */, A_YMIN = 12, A_YMAX, A_PAD0, A_PAD1 };

// f32 -> uint32 whose unsigned order is the floats' order (-inf lowest), and back
__host__ __device__ inline uint32_t fkey_bits(uint32_t b) { return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ inline uint32_t fkey(float v) { return fkey_bits(__float_as_uint(v)); }
__device__ inline uint32_t funkey_bits(uint32_t k) { return k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu); }
constexpr uint32_t kKeyPosInf = 0xFF800000u, kKeyNegInf = 0x007FFFFFu;      // fkey(+inf), fkey(-inf)

struct NoteArgs {
    PolarGrid G;
    uint32_t n_objects, extent_mask;
    int vec;                            // rows are read as 16-B label words and 4-B image words
    int occ_words, n_chunks;
};

// what a thread, a table entry or a merge holds of one object
struct Part {
    uint32_t id, nd, ng, nm, ne, bmin, bmax, xmin, xmax, ymin, ymax, sum, occ;
    unsigned long long peak;
};

__device__ inline void part_reset(Part& p, uint32_t id)
{
    p.id = id; p.nd = p.ng = p.nm = p.ne = 0;
    p.bmin = 0xFFFFFFFFu; p.bmax = 0; p.xmin = p.ymin = 0xFFFFFFFFu; p.xmax = p.ymax = 0; p.sum = 0; p.occ = 0; p.peak = 0;
}

// a partial record of a tile whose column 0 holds azimuth a0 into the accumulator and the occupancy row of record `rec`
__device__ inline void merge_global(uint32_t* acc_base, uint32_t* occ_base, size_t rec, const Part& p, int a0, const NoteArgs& A)
{
    uint32_t* acc = acc_base + rec * kAccWords;
    if (p.nd) atomicAdd(acc + A_ND, p.nd);
    if (p.ng) atomicAdd(acc + A_NG, p.ng);
    if (p.nm) atomicAdd(acc + A_NM, p.nm);
    if (!p.ne) return;
    atomicAdd(acc + A_NE, p.ne);
    atomicMin(acc + A_BMIN, p.bmin); atomicMax(acc + A_BMAX, p.bmax);
    atomicMin(acc + A_XMIN, p.xmin); atomicMax(acc + A_XMAX, p.xmax);
    atomicMin(acc + A_YMIN, p.ymin); atomicMax(acc + A_YMAX, p.ymax);
    atomicMax(reinterpret_cast<unsigned long long*>(acc + A_PEAK), p.peak);
    if (p.sum) atomicAdd(reinterpret_cast<unsigned long long*>(acc + A_SUM), (unsigned long long)p.sum);
    // tile column c holds azimuth a0 + c below `nowrap`, a0 + c - n_angles from there on
    uint32_t* row = occ_base + rec * (size_t)A.occ_words;
    const int nowrap = A.G.n_angles - a0;
    const uint32_t lo = nowrap >= 32 ? p.occ : p.occ & ((1u << nowrap) - 1u);
    const uint32_t hi = nowrap >= 32 ? 0u : p.occ >> nowrap;
    const unsigned long long w = (unsigned long long)lo << (a0 & 31);
    if ((uint32_t)w) atomicOr(row + (a0 >> 5), (uint32_t)w);
    if ((uint32_t)(w >> 32)) atomicOr(row + (a0 >> 5) + 1, (uint32_t)(w >> 32));
    if (hi) atomicOr(row, hi);
}

__global__ void __launch_bounds__(256) k_note_init(uint4* acc, size_t n_rec, uint32_t* occ, size_t n_occ, uint32_t* skipped, int n_frames)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = t; i < n_rec; i += step) {
        acc[4 * i + 0] = make_uint4(0u, 0u, 0u, 0u);
        acc[4 * i + 1] = make_uint4(0xFFFFFFFFu, 0u, kKeyPosInf, kKeyNegInf);
        acc[4 * i + 2] = make_uint4(0u, 0u, 0u, 0u);
        acc[4 * i + 3] = make_uint4(kKeyPosInf, kKeyNegInf, 0u, 0u);
    }
    for (size_t i = t; i < n_occ; i += step) occ[i] = 0u;
    if (t < (size_t)n_frames) skipped[t] = 0u;
}

__global__ void __launch_bounds__(kNoteTB) k_note_accum(const uint32_t* labels, const uint8_t* imgs, uint32_t* acc, uint32_t* occ, uint32_t* skipped,
                                                        NoteArgs A)
{
    __shared__ uint32_t t_key[kNoteSlots];
    __shared__ uint32_t t_w[12][kNoteSlots];       // nd ng nm ne bmin bmax xmin xmax ymin ymax sum occ
    __shared__ unsigned long long t_peak[kNoteSlots];
    __shared__ uint32_t s_skipped;

    for (int s = threadIdx.x; s < kNoteSlots; s += kNoteTB) {
        t_key[s] = kNoId;
        t_w[0][s] = t_w[1][s] = t_w[2][s] = t_w[3][s] = 0u;
        t_w[4][s] = 0xFFFFFFFFu; t_w[5][s] = 0u;
        t_w[6][s] = 0xFFFFFFFFu; t_w[7][s] = 0u; t_w[8][s] = 0xFFFFFFFFu; t_w[9][s] = 0u;
        t_w[10][s] = 0u; t_w[11][s] = 0u;
        t_peak[s] = 0ull;
    }
    if (threadIdx.x == 0) s_skipped = 0u;
    __syncthreads();

    const int f = blockIdx.y;
    const int tile = blockIdx.x / A.n_chunks, chunk = blockIdx.x - tile * A.n_chunks;
    const int col0 = tile * kNoteTW, row0 = chunk * kNoteRows, row_end = min(A.G.n_cells, row0 + kNoteRows);
    const int a0 = az_of_col(A.G, col0);
    const size_t rec0 = (size_t)f * A.n_objects;
    const int c0 = 4 * (threadIdx.x & 7), rr = threadIdx.x >> 3;

    bool valid[4];
    int az[4];
    float cs[4], sn[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
        valid[e] = col0 + c0 + e < A.G.n_angles;
        az[e] = a0 + c0 + e >= A.G.n_angles ? a0 + c0 + e - A.G.n_angles : a0 + c0 + e;
        const float theta = az_theta(A.G, az[e]);
        cs[e] = cosf(theta); sn[e] = sinf(theta);
    }

    // a partial record to the tile's table, or past a full table to the global atomics
    auto flush = [&](const Part& p) {
        if (p.id == kNoId) return;
        const uint32_t h = (p.id * 2654435761u) >> 25;
        int slot = -1;
        for (int k = 0; k < kNoteProbes; k++) {
            const int s = (int)((h + (uint32_t)k) & (uint32_t)(kNoteSlots - 1));
            const uint32_t old = atomicCAS(&t_key[s], kNoId, p.id);
            if (old == kNoId || old == p.id) { slot = s; break; }
        }
        if (slot < 0) { merge_global(acc, occ, rec0 + p.id, p, a0, A); return; }
        if (p.nd) atomicAdd(&t_w[0][slot], p.nd);
        if (p.ng) atomicAdd(&t_w[1][slot], p.ng);
        if (p.nm) atomicAdd(&t_w[2][slot], p.nm);
        if (!p.ne) return;
        atomicAdd(&t_w[3][slot], p.ne);
        atomicMin(&t_w[4][slot], p.bmin); atomicMax(&t_w[5][slot], p.bmax);
        atomicMin(&t_w[6][slot], p.xmin); atomicMax(&t_w[7][slot], p.xmax);
        atomicMin(&t_w[8][slot], p.ymin); atomicMax(&t_w[9][slot], p.ymax);
        if (p.sum) atomicAdd(&t_w[10][slot], p.sum);
        atomicOr(&t_w[11][slot], p.occ);
        atomicMax(&t_peak[slot], p.peak);
    };

    Part cur;
    part_reset(cur, kNoId);
    uint32_t n_skip = 0;
    const size_t plane = (size_t)f * A.G.n_cells * A.G.n_angles;
    for (int row = row0 + rr; row < row_end; row += kNoteTB / 8) {
        const size_t at = plane + (size_t)row * A.G.n_angles + col0 + c0;
        uint32_t lab[4] = { RR_LABEL_NONE, RR_LABEL_NONE, RR_LABEL_NONE, RR_LABEL_NONE };
        uint32_t z4 = 0;
        if (A.vec) {
            if (valid[0]) {             // n_angles is a multiple of 4: the four columns are there together
                const uint4 v = *reinterpret_cast<const uint4*>(labels + at);
                lab[0] = v.x; lab[1] = v.y; lab[2] = v.z; lab[3] = v.w;
                if (imgs) z4 = *reinterpret_cast<const uint32_t*>(imgs + at);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (valid[e]) {
                    lab[e] = labels[at + e];
                    if (imgs) z4 |= (uint32_t)imgs[at + e] << (8 * e);
                }
        }
        const float r = bin_range(A.G, row);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t L = lab[e];
            if (L == RR_LABEL_NONE) continue;
            const uint32_t id = L & 0xFFFFFFu;
            if (id >= A.n_objects) { n_skip++; continue; }
            if (id != cur.id) { flush(cur); part_reset(cur, id); }
            const uint32_t cls = ((L >> 28) & 1u) ? (uint32_t)RR_NOTE_MULTIPATH : ((L >> 24) & 15u) ? (uint32_t)RR_NOTE_GHOST : (uint32_t)RR_NOTE_DIRECT;
            cur.nd += cls == RR_NOTE_DIRECT; cur.ng += cls == RR_NOTE_GHOST; cur.nm += cls == RR_NOTE_MULTIPATH;
            if (cls & A.extent_mask) {
                const uint32_t z = (z4 >> (8 * e)) & 255u;
                const uint32_t kx = fkey(r * cs[e]), ky = fkey(r * sn[e]);
                cur.ne++;
                cur.bmin = min(cur.bmin, (uint32_t)row); cur.bmax = max(cur.bmax, (uint32_t)row);
                cur.xmin = min(cur.xmin, kx); cur.xmax = max(cur.xmax, kx);
                cur.ymin = min(cur.ymin, ky); cur.ymax = max(cur.ymax, ky);
                cur.sum += z;
                cur.occ |= 1u << (c0 + e);
                const unsigned long long key = ((unsigned long long)z << 32) | ((0xFFFFu - (uint32_t)row) << 16) | (0xFFFFu - (uint32_t)az[e]);
                cur.peak = key > cur.peak ? key : cur.peak;
            }
        }
    }
    flush(cur);
    if (n_skip) atomicAdd(&s_skipped, n_skip);
    __syncthreads();
    if (threadIdx.x == 0 && s_skipped) atomicAdd(skipped + f, s_skipped);
    for (int s = threadIdx.x; s < kNoteSlots; s += kNoteTB) {
        if (t_key[s] == kNoId) continue;
        Part p;
        p.id = t_key[s];
        p.nd = t_w[0][s]; p.ng = t_w[1][s]; p.nm = t_w[2][s]; p.ne = t_w[3][s];
        p.bmin = t_w[4][s]; p.bmax = t_w[5][s]; p.xmin = t_w[6][s]; p.xmax = t_w[7][s]; p.ymin = t_w[8][s]; p.ymax = t_w[9][s];
        p.sum = t_w[10][s]; p.occ = t_w[11][s]; p.peak = t_peak[s];
        merge_global(acc, occ, rec0 + p.id, p, a0, A);
    }
}

// a run of `len` unoccupied azimuths that begins at `start`: a longer run is a larger key, among equal runs the lower start
__device__ inline unsigned long long gap_key(int len, int start) { return ((unsigned long long)(uint32_t)len << 32) | (0xFFFFFFFFu - (uint32_t)start); }

__global__ void __launch_bounds__(256) k_note_finish(const uint32_t* acc_base, const uint32_t* occ_base, size_t n_rec, uint4* notes, int n_angles,
                                                     int occ_words)
{
    const int lane = threadIdx.x & (kNoteGroup - 1);
    const size_t g0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) / kNoteGroup, g_step = (size_t)gridDim.x * blockDim.x / kNoteGroup;
    for (size_t rec = g0; rec < n_rec; rec += g_step) {
        const uint32_t* row = occ_base + rec * (size_t)occ_words;
        unsigned long long best = 0ull;
        int first = -1, last = -1;          // the lowest and the highest occupied azimuth so far (the same in every lane of the group)
        for (int base = 0; base < occ_words; base += kNoteGroup) {
            const int wi = base + lane;
            const uint32_t w = wi < occ_words ? row[wi] : 0u;
            const int my_first = w ? wi * 32 + __ffs((int)w) - 1 : -1, my_last = w ? wi * 32 + 31 - __clz((int)w) : -1;
            int incl = my_last;             // the highest occupied azimuth up to and including this lane's word
            for (int d = 1; d < kNoteGroup; d <<= 1) {
                const int y = __shfl_up(incl, d, kNoteGroup);
                if (lane >= d) incl = max(incl, y);
            }
            int prev = __shfl_up(incl, 1, kNoteGroup);
            if (lane == 0) prev = -1;
            prev = max(prev, last);
            unsigned long long key = 0ull;
            if (w) {
                if (prev >= 0 && my_first - prev - 1 > 0) key = gap_key(my_first - prev - 1, prev + 1);
                int p = my_first;
                for (uint32_t t = w & (w - 1u); t; t &= t - 1u) {
                    const int q = wi * 32 + __ffs((int)t) - 1;
                    if (q - p - 1 > 0) { const unsigned long long k2 = gap_key(q - p - 1, p + 1); key = k2 > key ? k2 : key; }
                    p = q;
                }
            }
            int fmin = my_first < 0 ? 0x7FFFFFFF : my_first;
            for (int d = kNoteGroup / 2; d > 0; d >>= 1) {
                const unsigned long long k2 = __shfl_xor(key, d, kNoteGroup);
                key = k2 > key ? k2 : key;
                fmin = min(fmin, __shfl_xor(fmin, d, kNoteGroup));
            }
            best = key > best ? key : best;
            if (first < 0 && fmin != 0x7FFFFFFF) first = fmin;
            last = max(last, __shfl(incl, kNoteGroup - 1, kNoteGroup));
        }
        if (lane == 0) {                    // (the other lanes wait at the head of the loop: the next record's shuffles need the whole group)
            uint32_t az_begin = 0, az_count = 0;
            if (first >= 0) {
                const int len = first + n_angles - last - 1;        // the run through azimuth 0, or the two ends joined
                if (len > 0) { const unsigned long long k2 = gap_key(len, last + 1 == n_angles ? 0 : last + 1); best = k2 > best ? k2 : best; }
                if (best == 0ull) { az_begin = 0; az_count = (uint32_t)n_angles; }
                else {
                    const uint32_t glen = (uint32_t)(best >> 32), start = 0xFFFFFFFFu - (uint32_t)best;
                    az_begin = (start + glen) % (uint32_t)n_angles; az_count = (uint32_t)n_angles - glen;
                }
            }
            const uint4* a = reinterpret_cast<const uint4*>(acc_base + rec * kAccWords);
            const uint4 a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
            const bool any = a0.w != 0u;                            // n_extent
            const uint32_t peak = any ? a2.y : 0u, peak_bin = any ? 0xFFFFu - (a2.x >> 16) : 0u, peak_az = any ? 0xFFFFu - (a2.x & 0xFFFFu) : 0u;
            uint4* o = notes + rec * 5;
            o[0] = a0;
            o[1] = make_uint4(a1.x, a1.y, az_begin, az_count);
            o[2] = make_uint4(peak, peak_bin, peak_az, 0u);
            o[3] = make_uint4(a2.z, a2.w, funkey_bits(a1.z), funkey_bits(a1.w));
            o[4] = make_uint4(funkey_bits(a3.x), funkey_bits(a3.y), 0u, 0u);
        }
    }
}

// ---- the label under a detected point ----
__global__ void __launch_bounds__(256) k_label_points(const rr_radar_point* points, const uint32_t* offsets, int max_points, const uint32_t* labels,
                                                      const uint32_t* faces, const float* vel, uint32_t* p_labels, uint32_t* p_faces, float* p_vel,
                                                      int n_cells, int n_angles)
{
    const int f = blockIdx.y;
    const uint32_t total = offsets[(size_t)f * (n_angles + 1) + n_angles];
    const uint32_t m = min(total, (uint32_t)max_points);
    const size_t plane = (size_t)f * n_cells * n_angles, base = (size_t)f * max_points;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        const rr_radar_point p = points[base + i];
        const bool ok = p.bin < (uint32_t)n_cells && p.column < (uint32_t)n_angles;         // (a point that is not one of this shape names nothing)
        const size_t at = plane + (size_t)p.bin * n_angles + p.column;
        p_labels[base + i] = ok ? labels[at] : RR_LABEL_NONE;
        if (faces) p_faces[base + i] = ok ? faces[at] : RR_LABEL_NONE;
        if (vel) p_vel[base + i] = ok ? vel[at] : __uint_as_float(0x7FC00000u);
    }
}

// ---- Cartesian instance mask ----
struct CartLabelArgs { CartGrid C; PolarGrid G; };

// the nearest pixel of rr_detect.hip's k_cartesian (the same leaves of rr_polar.h); RR_LABEL_NONE beyond the last bin
__device__ inline uint32_t cart_label(const uint32_t* plane, const CartLabelArgs& A, int i, int j)
{
    const V3 p = pixel_xy(A.C, i, j);
    const float rho = sqrtf(p.x * p.x + p.y * p.y), phi = atan2f(p.y, p.x);
    float v;
    if (!range_coord(A.G, rho, &v)) return RR_LABEL_NONE;
    return polar_nearest(plane, A.G, az_coord(A.G, phi), v);
}

__global__ void __launch_bounds__(256) k_cartesian_labels(const uint32_t* planes, uint32_t* out, size_t total, CartLabelArgs A)
{
    const uint32_t w = (uint32_t)A.C.width, wsq = w * w;
    const size_t npx = (size_t)A.G.n_cells * A.G.n_angles;
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (size_t)gridDim.x * blockDim.x) {
        const size_t f = q / wsq;
        const uint32_t rem = (uint32_t)(q - f * wsq);
        const uint32_t i = rem / w, j = rem - i * w;
        out[q] = cart_label(planes + f * npx, A, (int)i, (int)j);
    }
}

inline int occ_words_of(int n_angles) { return (n_angles + 31) / 32; }

}  // namespace

// accumulators [n_frames][n_objects] of 64 bytes, then the occupancy rows [n_frames][n_objects][ceil(n_angles / 32)] words, a multiple of 16 bytes
size_t note_scratch_bytes(size_t n_frames, size_t n_objects, int n_angles)
{
    const size_t n_rec = n_frames * n_objects;
    return (n_rec * (kAccWords * 4 + (size_t)occ_words_of(n_angles) * 4) + 15) & ~(size_t)15;
}

void launch_notes(const uint32_t* labels, const uint8_t* imgs, int n_frames, uint32_t n_objects, uint32_t extent_mask, const PolarGrid& G,
                  rr_object_note* notes, uint32_t* skipped, void* scratch, hipStream_t s)
{
    const int n_cells = G.n_cells, n_angles = G.n_angles;
    NoteArgs A;
    A.G = G;
    A.n_objects = n_objects; A.extent_mask = extent_mask;
    A.vec = n_angles % 4 == 0 && reinterpret_cast<uintptr_t>(labels) % 16 == 0 && reinterpret_cast<uintptr_t>(imgs) % 4 == 0;
    A.occ_words = occ_words_of(n_angles); A.n_chunks = (n_cells + kNoteRows - 1) / kNoteRows;
    const size_t n_rec = (size_t)n_frames * n_objects, n_occ = n_rec * (size_t)A.occ_words;
    uint32_t* acc = static_cast<uint32_t*>(scratch);
    uint32_t* occ = acc + n_rec * kAccWords;
    const unsigned init_groups = (unsigned)std::min<size_t>((std::max(n_occ, n_rec) + 255) / 256, 16384);
    hipLaunchKernelGGL(k_note_init, dim3(init_groups), dim3(256), 0, s, reinterpret_cast<uint4*>(acc), n_rec, occ, n_occ, skipped, n_frames);
    const dim3 grid((unsigned)(((n_angles + kNoteTW - 1) / kNoteTW) * A.n_chunks), (unsigned)n_frames);
    hipLaunchKernelGGL(k_note_accum, grid, dim3(kNoteTB), 0, s, labels, imgs, acc, occ, skipped, A);
    const unsigned fin_groups = (unsigned)std::min<size_t>((n_rec * kNoteGroup + 255) / 256, 65536);
    hipLaunchKernelGGL(k_note_finish, dim3(fin_groups), dim3(256), 0, s, (const uint32_t*)acc, (const uint32_t*)occ, n_rec, reinterpret_cast<uint4*>(notes),
                       n_angles, A.occ_words);
}

void launch_label_points(const rr_radar_point* points, const uint32_t* offsets, int n_frames, int max_points, const uint32_t* labels, const uint32_t* faces,
                         const float* vel, uint32_t* p_labels, uint32_t* p_faces, float* p_vel, int n_cells, int n_angles, hipStream_t s)
{
    const dim3 grid((unsigned)std::min(1024, (max_points + 255) / 256), (unsigned)n_frames);
    hipLaunchKernelGGL(k_label_points, grid, dim3(256), 0, s, points, offsets, max_points, labels, faces, vel, p_labels, p_faces, p_vel, n_cells, n_angles);
}

void launch_cartesian_labels(const uint32_t* planes, int n_frames, const rr_cartesian_config& cfg, const PolarGrid& G, uint32_t* out, hipStream_t s)
{
    const CartLabelArgs A = { { cfg.width, cfg.pixel_size }, G };
    const size_t total = (size_t)n_frames * cfg.width * cfg.width;
    const size_t groups = std::min<size_t>((total + 255) / 256, 16384);
    hipLaunchKernelGGL(k_cartesian_labels, dim3((unsigned)groups), dim3(256), 0, s, planes, out, total, A);
}

}  // namespace rr
