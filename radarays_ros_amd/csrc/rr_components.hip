// rr_components.hip -- gfx950 kernels that label the connected components of thresholded uint8 planes (rr_label_components_device): the
// clusters of a polar image (a cylinder: the column axis may wrap) and the segments of a grid map.  The definition is in
// include/radarays_mi355.h: a component's label is the smallest linear index in it, so no execution order can change a byte.
//
//   k_cc_tile      one workgroup per tile of kCcTW x kCcTH pixels: union-find over the tile in LDS (a pixel is united with its left, upper
//                  and, at 8-connectivity, upper diagonal neighbours inside the tile), then every pixel's tile root goes to the link plane
//                  as a linear index of the plane; background is RR_LABEL_NONE.  Zeroes the count plane
//   k_cc_border    one thread per pixel of the first row of a tile row and of the first column of a tile column (and of column 0 under
//                  wrap_x): the pairs of neighbours across tile borders and across the seam, united in the link plane
//   k_cc_flatten   a launch of its own: the launch boundary before it makes every link of k_cc_border visible.  Every pixel follows its
//                  links to the root, stores it, and counts itself at the root's position (reduced over the wave's runs of equal roots)
//   k_cc_partial   per chunk of kCcChunk pixels the number of kept roots (count >= min_pixels) and of dropped roots
//   k_cc_offsets   one workgroup per plane: the exclusive scan of the chunks' kept numbers in place, the plane's two totals to d_counts
//   k_cc_rank      per chunk again: every root's rank in ascending root order over the count plane (RR_LABEL_NONE for a dropped root), and
//                  the identity of the accumulators of every record that will be written
//   k_cc_emit      every pixel: the label and the cleaned value, and, reduced over the wave's runs of equal rank before any atomic, the
//                  pixel into its component's record (integers only: add, min, max, or, one packed 64-bit max key for the peak)
//   k_cc_finish    a thread per written record: the peak key unpacked, col_lo_max brought from its biased form, the record in five 16-B stores
//
// The merge is safe where workgroups share a machine: no workgroup waits for another (no spin, no flag, no pass repeated until nothing
// changes); a link only ever points to a smaller or equal index, so a find ends after at most as many steps as its start index; unite()
// lowers the larger root with a device-scope atomicMin, goes on from the value the atomic returned and ends when the roots agree; every
// read of a link that another workgroup may change in the same launch is an agent-scope atomic load (the L2s of different XCDs are not
// coherent within a launch: MI355X_MICROARCH.md, inter-workgroup visibility), and a stale link is an older ancestor: it costs steps, never
// the answer.  Only the launch boundary before k_cc_flatten is relied on for visibility.
// Rests on: partial reduction on chip before any global atomic (cdna_hip_programming.md, Guideline 12; every workgroup adding into one row
// is the measured worst case, MI355X_MICROARCH.md, atomics table); wave64 shuffles.  Every value travels as a kernel argument; all working
// memory is the caller's scratch; the kernels use no scratch (private) memory and 4 KB of static LDS.
#include "../../include/radarays_mi355.h"
#include "rr_device.h"
#include "rr_launch.h"

#include <algorithm>

namespace rr {

namespace {

constexpr int kCcTW = 64, kCcTH = 16;           // a tile: one wave per row sweep, 1024 links of LDS
constexpr int kCcTB = 256;                      // threads of a workgroup of every kernel here
constexpr int kCcTile = kCcTW * kCcTH;
constexpr int kCcPer = 4;                       // consecutive pixels of a thread of k_cc_partial / k_cc_rank
constexpr int kCcChunk = kCcTB * kCcPer;        // pixels of a chunk of the scan
constexpr uint32_t kNone = RR_LABEL_NONE;

struct CcArgs {
    int H, W, n_planes;
    uint32_t npx;                               // H * W <= 2^26
    uint32_t threshold, min_pixels, max_components;
    int conn8, wrap;
    int tiles_x, tiles_y;
    uint32_t n_chunks;
};

#define CC_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// ---- union-find in LDS (k_cc_tile): links are tile-local indices, all accesses volatile or atomic ----
__device__ inline uint32_t find_lds(volatile uint32_t* link, uint32_t x)
{
    for (uint32_t q; (q = link[x]) != x;) x = q;          // q < x: at most x steps
    return x;
}

__device__ inline void unite_lds(uint32_t* link, uint32_t a, uint32_t b)
{
    for (;;) {
        a = find_lds(link, a); b = find_lds(link, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(&link[a], b);
        if (old == a) return;                             // a was a root and now hangs under b
        a = old;                                          // a had been given another parent meanwhile: that one and b are still to be joined
    }
}

// ---- union-find in the link plane (k_cc_border, k_cc_flatten) ----
__device__ inline uint32_t ld_link(const uint32_t* p) { return __hip_atomic_load(p, CC_RLX_AGENT); }

__device__ inline uint32_t find_global(const uint32_t* link, uint32_t x)
{
    for (uint32_t q; (q = ld_link(link + x)) != x;) x = q;
    return x;
}

// ... and every link on the way lowered to the root that was found (an ancestor, so the links stay what they were: ancestors that only
// decrease): the chains through tile roots stay short on a plane whose components span thousands of tiles
__device__ inline uint32_t find_compress(uint32_t* link, uint32_t x)
{
    const uint32_t r = find_global(link, x);
    for (uint32_t y = x; y > r;) {                        // y falls strictly: at most x steps
        const uint32_t next = ld_link(link + y);
        if (next == y) break;
        if (next > r) __hip_atomic_fetch_min(link + y, r, CC_RLX_AGENT);
        y = next;
    }
    return r;
}

__device__ inline void unite_global(uint32_t* link, uint32_t a, uint32_t b)
{
    for (;;) {
        a = find_compress(link, a); b = find_compress(link, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = __hip_atomic_fetch_min(link + a, b, CC_RLX_AGENT);
        if (old == a) return;
        a = old;
    }
}

__global__ void __launch_bounds__(kCcTB) k_cc_tile(const uint8_t* planes, uint32_t* links, uint32_t* counts, CcArgs A)
{
    __shared__ uint32_t s_link[kCcTile];
    const int ty = blockIdx.x / A.tiles_x, tx = blockIdx.x - ty * A.tiles_x;
    const int x0 = tx * kCcTW, y0 = ty * kCcTH;
    const size_t base = (size_t)blockIdx.y * A.npx;
#pragma unroll
    for (int k = 0; k < kCcTile / kCcTB; k++) {
        const int li = k * kCcTB + threadIdx.x, lx = li & (kCcTW - 1), ly = li / kCcTW;
        const int gx = x0 + lx, gy = y0 + ly;
        bool fg = false;
        if (gx < A.W && gy < A.H) {
            const size_t at = base + (size_t)gy * A.W + gx;
            fg = planes[at] >= A.threshold;
            counts[at] = 0u;
        }
        s_link[li] = fg ? (uint32_t)li : kNone;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kCcTile / kCcTB; k++) {
        const int li = k * kCcTB + threadIdx.x, lx = li & (kCcTW - 1), ly = li / kCcTW;
        volatile uint32_t* v = s_link;
        if (v[li] == kNone) continue;
        // (whether a neighbour is foreground never changes: a link is RR_LABEL_NONE or an index for good)
        if (lx > 0 && v[li - 1] != kNone) unite_lds(s_link, li, li - 1);
        if (ly > 0) {
            const bool up = v[li - kCcTW] != kNone;
            if (up) unite_lds(s_link, li, li - kCcTW);
            else if (A.conn8) {                                     // (with the upper pixel set, both diagonals hang on it already)
                if (lx > 0 && v[li - kCcTW - 1] != kNone) unite_lds(s_link, li, li - kCcTW - 1);
                if (lx < kCcTW - 1 && v[li - kCcTW + 1] != kNone) unite_lds(s_link, li, li - kCcTW + 1);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kCcTile / kCcTB; k++) {
        const int li = k * kCcTB + threadIdx.x, lx = li & (kCcTW - 1), ly = li / kCcTW;
        const int gx = x0 + lx, gy = y0 + ly;
        if (gx >= A.W || gy >= A.H) continue;
        uint32_t root = kNone;
        if (s_link[li] != kNone) {
            const uint32_t r = find_lds(s_link, li);
            root = (uint32_t)(y0 + (int)(r / kCcTW)) * (uint32_t)A.W + (uint32_t)(x0 + (int)(r & (kCcTW - 1)));   // row-major in the tile and in the plane: the order holds
        }
        links[base + (size_t)gy * A.W + gx] = root;
    }
}

// items of a plane: first (tiles_y - 1) * W pixels of the rows that begin a tile row, then (tiles_x - 1 + wrap) * H pixels of the columns
// that begin a tile column (column 0 last, under wrap_x: its left neighbour is column W - 1)
__global__ void __launch_bounds__(kCcTB) k_cc_border(const uint8_t* planes, uint32_t* links, CcArgs A, uint32_t n_rows_items, uint32_t n_items)
{
    const uint32_t item = blockIdx.x * kCcTB + threadIdx.x;
    if (item >= n_items) return;
    const size_t base = (size_t)blockIdx.y * A.npx;
    const uint8_t* plane = planes + base;
    uint32_t* link = links + base;
    const int W = A.W, H = A.H;
    auto fg = [&](int r, int c) { return plane[(size_t)r * W + c] >= A.threshold; };
    auto at = [&](int r, int c) { return (uint32_t)r * (uint32_t)W + (uint32_t)c; };
    if (item < n_rows_items) {
        const int r = ((int)(item / (uint32_t)W) + 1) * kCcTH, c = (int)(item % (uint32_t)W);
        if (!fg(r, c)) return;
        if (fg(r - 1, c)) { unite_global(link, at(r, c), at(r - 1, c)); return; }       // (both upper diagonals hang on the upper pixel)
        if (!A.conn8) return;
        const int cl = c > 0 ? c - 1 : (A.wrap ? W - 1 : -1), cr = c < W - 1 ? c + 1 : (A.wrap ? 0 : -1);
        if (cl >= 0 && fg(r - 1, cl)) unite_global(link, at(r, c), at(r - 1, cl));
        if (cr >= 0 && fg(r - 1, cr)) unite_global(link, at(r, c), at(r - 1, cr));
    } else {
        const uint32_t j = item - n_rows_items;
        const int k = (int)(j / (uint32_t)H), r = (int)(j % (uint32_t)H);
        const int c = k < A.tiles_x - 1 ? (k + 1) * kCcTW : 0, cl = c > 0 ? c - 1 : W - 1;
        if (!fg(r, c)) return;
        if (fg(r, cl)) unite_global(link, at(r, c), at(r, cl));
        if (!A.conn8) return;
        if (r > 0 && fg(r - 1, cl)) unite_global(link, at(r, c), at(r - 1, cl));
        if (r < H - 1 && fg(r + 1, cl)) unite_global(link, at(r, c), at(r + 1, cl));
    }
}

// the lanes of a wave hold consecutive pixels: a run is a stretch of lanes with the same key.  run_id: which run a lane is in; head: its first lane
__device__ inline int run_of(uint32_t key, bool& head)
{
    const int lane = threadIdx.x & 63;
    const uint32_t prev = __shfl_up(key, 1, 64);
    head = lane == 0 || prev != key;
    const unsigned long long heads = __ballot(head);
    return __builtin_popcountll(heads & (~0ull >> (63 - lane)));
}

// x reduced over the lanes of the caller's run from this lane upwards (the run's head gets the run's value): op is add, min or max
template <class T, class Op> __device__ inline T run_reduce(T x, int run, Op op)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T y = __shfl_down(x, off, 64);
        const int r = __shfl_down(run, off, 64);
        if (lane + off < 64 && r == run) x = op(x, y);
    }
    return x;
}

__global__ void __launch_bounds__(kCcTB) k_cc_flatten(uint32_t* links, uint32_t* counts, CcArgs A)
{
    const size_t base = (size_t)blockIdx.y * A.npx;
    uint32_t* link = links + base;
    const uint32_t p = blockIdx.x * kCcTB + threadIdx.x;          // (a whole wave is in or out of the plane together only by accident: no early return)
    uint32_t root = kNone;
    if (p < A.npx && ld_link(link + p) != kNone) {
        root = find_global(link, p);
        __hip_atomic_store(link + p, root, CC_RLX_AGENT);         // (another pixel's find may pass through here: the old parent and the root are both ancestors)
    }
    if (__ballot(root != kNone) == 0ull) return;
    bool head;
    const int run = run_of(root, head);
    const uint32_t n = run_reduce((uint32_t)(root != kNone), run, [](uint32_t a, uint32_t b) { return a + b; });
    if (head && root != kNone) atomicAdd(counts + base + root, n);
}

__device__ inline void root_flags(const uint32_t* link, const uint32_t* counts, uint32_t p, const CcArgs& A, int& keep, int& drop)
{
    keep = drop = 0;
    if (p < A.npx && link[p] == p) { keep = counts[p] >= A.min_pixels; drop = !keep; }
}

__global__ void __launch_bounds__(kCcTB) k_cc_partial(const uint32_t* links, const uint32_t* counts, uint32_t* partials, CcArgs A)
{
    __shared__ int s_scan[8];
    const size_t base = (size_t)blockIdx.y * A.npx;
    const uint32_t p0 = blockIdx.x * kCcChunk + threadIdx.x * kCcPer;
    int nk = 0, nd = 0;
#pragma unroll
    for (int e = 0; e < kCcPer; e++) {
        int k, d;
        root_flags(links + base, counts + base, p0 + e, A, k, d);
        nk += k; nd += d;
    }
    int tk, td;
    block_excl_scan(nk, tk, s_scan);
    block_excl_scan(nd, td, s_scan);
    if (threadIdx.x == 0) {
        uint32_t* out = partials + ((size_t)blockIdx.y * A.n_chunks + blockIdx.x) * 2;
        out[0] = (uint32_t)tk; out[1] = (uint32_t)td;
    }
}

__global__ void __launch_bounds__(kCcTB) k_cc_offsets(uint32_t* partials, uint32_t* totals, CcArgs A)
{
    __shared__ int s_scan[8];
    uint32_t* part = partials + (size_t)blockIdx.x * A.n_chunks * 2;
    int carry = 0, dropped = 0;
    for (uint32_t c0 = 0; c0 < A.n_chunks; c0 += kCcTB) {         // (the bound is the same in every thread: the barriers inside are met by all)
        const uint32_t c = c0 + threadIdx.x;
        const int k = c < A.n_chunks ? (int)part[2 * c] : 0, d = c < A.n_chunks ? (int)part[2 * c + 1] : 0;
        int tk, td;
        const int ex = block_excl_scan(k, tk, s_scan);
        block_excl_scan(d, td, s_scan);
        if (c < A.n_chunks) part[2 * c] = (uint32_t)(carry + ex);
        carry += tk; dropped += td;
    }
    if (threadIdx.x == 0) { totals[2 * blockIdx.x] = (uint32_t)carry; totals[2 * blockIdx.x + 1] = (uint32_t)dropped; }
}

// the accumulators of a record, in its own 80 bytes (words): root, n_pixels, row_min, row_max | col_min, col_max, col_lo_max + 1, col_hi_min |
// the peak key (u64), -, flags | sum_intensity, sum_row | sum_col, reserved_
__global__ void __launch_bounds__(kCcTB) k_cc_rank(const uint32_t* links, uint32_t* counts, const uint32_t* partials, uint4* comps, CcArgs A)
{
    __shared__ int s_scan[8];
    const size_t base = (size_t)blockIdx.y * A.npx;
    const uint32_t p0 = blockIdx.x * kCcChunk + threadIdx.x * kCcPer;
    int keep[kCcPer], drop[kCcPer], nk = 0;
#pragma unroll
    for (int e = 0; e < kCcPer; e++) { root_flags(links + base, counts + base, p0 + e, A, keep[e], drop[e]); nk += keep[e]; }
    int total;
    uint32_t rank = partials[((size_t)blockIdx.y * A.n_chunks + blockIdx.x) * 2] + (uint32_t)block_excl_scan(nk, total, s_scan);
#pragma unroll
    for (int e = 0; e < kCcPer; e++) {
        if (drop[e]) counts[base + p0 + e] = kNone;
        if (!keep[e]) continue;
        counts[base + p0 + e] = rank;
        if (rank < A.max_components) {
            uint4* o = comps + ((size_t)blockIdx.y * A.max_components + rank) * 5;
            o[0] = make_uint4(p0 + e, 0u, kNone, 0u);
            o[1] = make_uint4(kNone, 0u, 0u, kNone);
            o[2] = make_uint4(0u, 0u, 0u, 0u);
            o[3] = make_uint4(0u, 0u, 0u, 0u);
            o[4] = make_uint4(0u, 0u, 0u, 0u);
        }
        rank++;
    }
}

__global__ void __launch_bounds__(kCcTB) k_cc_emit(const uint8_t* planes, const uint32_t* links, const uint32_t* ranks, uint32_t* labels, uint8_t* clean,
                                                   uint32_t* comps, CcArgs A)
{
    const size_t base = (size_t)blockIdx.y * A.npx;
    const uint32_t p = blockIdx.x * kCcTB + threadIdx.x;
    uint32_t value = 0, root = kNone, rank = kNone;
    if (p < A.npx) {
        value = planes[base + p];
        if (value >= A.threshold) { root = links[base + p]; rank = ranks[base + root]; }
        const bool kept = rank != kNone;
        if (labels) labels[base + p] = kept ? root : kNone;       // (in place over the link plane: a thread reads and writes its own pixel only)
        if (clean) clean[base + p] = kept ? (uint8_t)value : (uint8_t)0;
    }
    const uint32_t key = rank < A.max_components ? rank : kNone;  // (kNone is no rank: max_components is below 2^31)
    if (__ballot(key != kNone) == 0ull) return;

    const uint32_t W = (uint32_t)A.W, H = (uint32_t)A.H;
    const uint32_t row = p / W, col = p - row * W;
    uint32_t flags = 0;
    if (key != kNone) {
        const uint8_t* plane = planes + base;
        if (row == 0 || row == H - 1 || (!A.wrap && (col == 0 || col == W - 1))) flags |= RR_COMP_BORDER;
        if (A.wrap && col == 0) {                                 // (a pair across the seam is seen from its column-0 side: one component holds both)
            bool seam = plane[(size_t)row * W + W - 1] >= A.threshold;
            if (A.conn8) {
                if (row > 0) seam = seam || plane[(size_t)(row - 1) * W + W - 1] >= A.threshold;
                if (row < H - 1) seam = seam || plane[(size_t)(row + 1) * W + W - 1] >= A.threshold;
            }
            if (seam) flags |= RR_COMP_SEAM;
        }
    }
    bool head;
    const int run = run_of(key, head);
    auto add = [](auto a, auto b) { return a + b; };
    auto mn = [](auto a, auto b) { return a < b ? a : b; };
    auto mx = [](auto a, auto b) { return a > b ? a : b; };
    const bool lo = col < W / 2;
    const uint32_t n = run_reduce(1u, run, add);
    const uint32_t row_min = run_reduce(row, run, mn), row_max = run_reduce(row, run, mx);
    const uint32_t col_min = run_reduce(col, run, mn), col_max = run_reduce(col, run, mx);
    const uint32_t lo_max = run_reduce(lo ? col + 1u : 0u, run, mx), hi_min = run_reduce(lo ? kNone : col, run, mn);
    const unsigned long long peak = run_reduce(((unsigned long long)value << 32) | (unsigned long long)(~p), run, mx);
    const uint32_t fl = run_reduce(flags, run, [](uint32_t a, uint32_t b) { return a | b; });
    const uint32_t sum_v = run_reduce(value, run, add), sum_r = run_reduce(row, run, add), sum_c = run_reduce(col, run, add);
    if (!head || key == kNone) return;
    uint32_t* o = comps + ((size_t)blockIdx.y * A.max_components + key) * 20;
    unsigned long long* o64 = reinterpret_cast<unsigned long long*>(o);
    atomicAdd(o + 1, n);
    atomicMin(o + 2, row_min); atomicMax(o + 3, row_max);
    atomicMin(o + 4, col_min); atomicMax(o + 5, col_max);
    if (lo_max) atomicMax(o + 6, lo_max);
    if (hi_min != kNone) atomicMin(o + 7, hi_min);
    atomicMax(o64 + 4, peak);
    if (fl) atomicOr(o + 11, fl);
    atomicAdd(o64 + 6, (unsigned long long)sum_v);
    atomicAdd(o64 + 7, (unsigned long long)sum_r);
    atomicAdd(o64 + 8, (unsigned long long)sum_c);
}

__global__ void __launch_bounds__(kCcTB) k_cc_finish(uint4* comps, const uint32_t* totals, CcArgs A)
{
    const uint32_t kept = totals[2 * blockIdx.y], n = kept < A.max_components ? kept : A.max_components;
    for (uint32_t i = blockIdx.x * kCcTB + threadIdx.x; i < n; i += gridDim.x * kCcTB) {
        uint4* o = comps + ((size_t)blockIdx.y * A.max_components + i) * 5;
        const uint4 a1 = o[1], a2 = o[2];
        const uint32_t at = ~a2.x;                                // the key's low word: the complement of the peak's linear index
        o[1] = make_uint4(a1.x, a1.y, a1.z - 1u, a1.w);           // (0 - 1: RR_LABEL_NONE, no column below W / 2)
        o[2] = make_uint4(a2.y, at / (uint32_t)A.W, at % (uint32_t)A.W, a2.w);
    }
}

inline uint32_t chunks_of(size_t npx) { return (uint32_t)((npx + kCcChunk - 1) / kCcChunk); }
inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

}  // namespace

void components_tile_sizes(int* tile_w, int* tile_h) { if (tile_w) *tile_w = kCcTW; if (tile_h) *tile_h = kCcTH; }

// the link plane (used when the caller gives no label plane), the count / rank plane, the scan partials: each a multiple of 16 bytes
size_t components_scratch_bytes(size_t n_planes, size_t npx)
{
    return 2 * up16(n_planes * npx * 4) + up16(n_planes * chunks_of(npx) * 8);
}

void launch_components(const uint8_t* planes, int n_planes, const rr_components_config& cfg, uint32_t* labels, uint8_t* clean, rr_component* comps,
                       uint32_t* totals, void* scratch, hipStream_t s)
{
    CcArgs A;
    A.H = cfg.height; A.W = cfg.width; A.n_planes = n_planes;
    A.npx = (uint32_t)cfg.height * (uint32_t)cfg.width;
    A.threshold = (uint32_t)cfg.threshold; A.min_pixels = (uint32_t)cfg.min_pixels; A.max_components = (uint32_t)cfg.max_components;
    A.conn8 = cfg.connectivity == 8; A.wrap = cfg.wrap_x != 0;
    A.tiles_x = (A.W + kCcTW - 1) / kCcTW; A.tiles_y = (A.H + kCcTH - 1) / kCcTH;
    A.n_chunks = chunks_of(A.npx);
    const size_t plane_bytes = up16((size_t)n_planes * A.npx * 4);
    uint8_t* sc = static_cast<uint8_t*>(scratch);
    uint32_t* links = labels ? labels : reinterpret_cast<uint32_t*>(sc);
    uint32_t* counts = reinterpret_cast<uint32_t*>(sc + plane_bytes);
    uint32_t* partials = reinterpret_cast<uint32_t*>(sc + 2 * plane_bytes);
    const unsigned ny = (unsigned)n_planes, px_groups = (A.npx + kCcTB - 1) / kCcTB;

    hipLaunchKernelGGL(k_cc_tile, dim3((unsigned)(A.tiles_x * A.tiles_y), ny), dim3(kCcTB), 0, s, planes, links, counts, A);
    const uint32_t n_rows_items = (uint32_t)(A.tiles_y - 1) * (uint32_t)A.W;
    const uint32_t n_items = n_rows_items + (uint32_t)(A.tiles_x - 1 + A.wrap) * (uint32_t)A.H;
    if (n_items)
        hipLaunchKernelGGL(k_cc_border, dim3((n_items + kCcTB - 1) / kCcTB, ny), dim3(kCcTB), 0, s, planes, links, A, n_rows_items, n_items);
    hipLaunchKernelGGL(k_cc_flatten, dim3(px_groups, ny), dim3(kCcTB), 0, s, links, counts, A);
    hipLaunchKernelGGL(k_cc_partial, dim3(A.n_chunks, ny), dim3(kCcTB), 0, s, (const uint32_t*)links, (const uint32_t*)counts, partials, A);
    hipLaunchKernelGGL(k_cc_offsets, dim3(ny), dim3(kCcTB), 0, s, partials, totals, A);
    hipLaunchKernelGGL(k_cc_rank, dim3(A.n_chunks, ny), dim3(kCcTB), 0, s, (const uint32_t*)links, counts, (const uint32_t*)partials,
                       reinterpret_cast<uint4*>(comps), A);
    if (labels || clean || A.max_components)
        hipLaunchKernelGGL(k_cc_emit, dim3(px_groups, ny), dim3(kCcTB), 0, s, planes, (const uint32_t*)links, (const uint32_t*)counts, labels, clean,
                           reinterpret_cast<uint32_t*>(comps), A);
    if (A.max_components) {
        const unsigned groups = (unsigned)std::min<uint32_t>((std::min(A.max_components, A.npx) + kCcTB - 1) / kCcTB, 1024u);
        hipLaunchKernelGGL(k_cc_finish, dim3(groups, ny), dim3(kCcTB), 0, s, reinterpret_cast<uint4*>(comps), (const uint32_t*)totals, A);
    }
}

}  // namespace rr
