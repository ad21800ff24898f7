// rr_labels.hip -- echo provenance (rr_simulate_batch_provenance_device, rr_debug_labels; the definition of a label is in
// include/radarays_mi355.h).  k_shade knows the triangle, its object and the pass when it writes an echo into a wave's slot; the next
// pass' k_trace overwrites hit[] and the link is gone.  These kernels keep it, beside a frame chain whose own kernels do not change:
//
//   k_echo_gather  behind the k_shade launch of EVERY pass, one workgroup per segment: walks the pass' slots in slot order and appends
//                  every echo (cell >= 0) to the segment's list at echo_count[seg] + its stable prefix within the pass (block_excl_scan,
//                  as k_scan compacts), tagged with the face and object of the triangle its wave hit, the pass and the kind (odd slot =
//                  multipath echo).  Slot order within a pass, passes in sequence: the order of k_scan's compacted list followed by
//                  k_column's staging of the last pass = the reference's order.  The last pass' odd slots exist only with
//                  record_multi_path (k_shade<., LAST> does not write them otherwise) and are read only then: k_column's sl_sh rule.
//                  Pass 0 writes echo_count, later passes advance it: no memset in the chain.  Reads count, sigtmp, hit, tris.
//   k_label        once, behind k_column, one workgroup per segment: the column as uint64 keys in LDS (dynamic, 8 B per cell: 27 KB at
//                  3,424 cells, 64 KB at the limit of 8,192), zeroed; every (echo, tap) pair of the segment is one work item, taps fastest,
//                  so the lanes of a wave hit neighbouring bins (consecutive LDS words, no bank conflict inside an echo's window); an item
//                  folds key = bits(term) << 32 | ~echo index into its bin with a 64-bit LDS atomic max.  Max is order-free: the result
//                  does not depend on scheduling.  Then key -> echo -> (info, face), two coalesced columns.
//   k_echo_export  the lists -> the caller's [segment][echo_stride] records and true counts (the first echo_stride echoes of a longer list)
//
// The term is (float)((double)strength * (double)w[tap]): the product is exact in f64 (24 x 24 bits), one rounding; this file is built
// with -ffp-contract=off like the rest.  No kernel uses scratch; k_echo_gather 288 B of static LDS (the scan's 32 and the barrier's vote), k_label dynamic LDS only.
#include "../../include/radarays_mi355.h"
#include "rr_device.h"
#include "rr_launch.h"

namespace rr {

static_assert(sizeof(EchoSrc) == sizeof(rr_echo_src) && sizeof(EchoSrc) == 16, "the lists are exported as they lie");
static_assert(kNoLabel == RR_LABEL_NONE && kLabelMaxCells == RR_LABEL_MAX_CELLS, "the header states the kernels' constants");

// grid n_seg, block 256
__global__ __launch_bounds__(256) void k_echo_gather(const Params P, const int pass)
{
    __shared__ int lds[8];
    const int seg = blockIdx.x;
    const int count = pass == 0 ? P.n_beam : (int)P.count[pass & 1][seg];
    // a wave owns two slots; the last pass' odd ones are written only with record_multi_path: entry e = slot e << sl_sh
    const int sl_sh = (pass == P.n_passes - 1 && !P.record_multi_path) ? 1 : 0;
    const int n_entries = (2 * count) >> sl_sh;
    const size_t base2 = (size_t)seg * 2 * P.cap;
    EchoSrc* out = P.prov + (size_t)seg * P.prov_cap;
    uint32_t n = pass == 0 ? 0u : P.prov_count[seg];
    int ovf = 0;
    for (int b = 0; b < n_entries; b += 256) {
        const int e = b + (int)threadIdx.x;
        const int sl = e << sl_sh;
        SigRec r = { -1, 0.0f };
        if (e < n_entries) r = P.sigtmp[base2 + sl];
        const int g = r.cell >= 0 ? 1 : 0;
        int tot;
        const int pre = block_excl_scan(g, tot, lds);
        if (g) {
            const uint32_t pos = n + (uint32_t)pre;
            if (pos < (uint32_t)P.prov_cap) {
                // the wave of slots 2j, 2j + 1 is entry j of the pass' hit list; an echo means it hit
                const uint32_t tri = P.hit[(size_t)seg * P.cap + (sl >> 1)].y;
                const float4* tp = reinterpret_cast<const float4*>(P.tris + tri);
                EchoSrc o;
                o.cell = r.cell; o.strength = r.strength;
                o.face = __float_as_uint(tp[0].w);
                o.info = (__float_as_uint(tp[1].w) & 0xFFFFFFu) | ((uint32_t)pass << 24) | ((uint32_t)(sl & 1) << 28);
                out[pos] = o;
            } else ovf = 1;         // (impossible by the size of the list: guarded anyway)
        }
        n += (uint32_t)tot;
    }
    if (__syncthreads_or(ovf) && threadIdx.x == 0) { atomicOr(&P.counters->overflow, 1u); atomicOr(P.sticky, 1u); }
    if (threadIdx.x == 0) P.prov_count[seg] = n;
}

// grid n_seg, block 256, dynamic LDS 8 B x n_cells.  w null: no denoiser (W = 1, mode = 0, weight 1)
__global__ __launch_bounds__(256) void k_label(const EchoSrc* __restrict__ lists, const uint32_t* __restrict__ counts, const size_t stride,
                                               const int n_cells, const int W, const int mode, const float* __restrict__ w,
                                               uint32_t* __restrict__ label_cols, uint32_t* __restrict__ face_cols)
{
    extern __shared__ unsigned long long s_key[];       // [n_cells] 0: nobody reached the bin
    const int seg = blockIdx.x;
    const EchoSrc* list = lists + (size_t)seg * stride;
    const uint32_t n = (uint32_t)min((size_t)counts[seg], stride);
    for (int g = threadIdx.x; g < n_cells; g += 256) s_key[g] = 0ull;
    __syncthreads();
    // item i = k * W + tap; this thread takes i = tid, tid + 256, ...: (k, tap) advance by (256 / W, 256 % W) with a carry
    const uint32_t dk = 256u / (uint32_t)W, dt = 256u % (uint32_t)W;
    uint32_t k = threadIdx.x / (uint32_t)W, tap = threadIdx.x % (uint32_t)W;
    while (k < n) {
        const EchoSrc r = list[k];
        if (r.cell >= 0 && r.cell < n_cells) {
            const int g = r.cell - mode + (int)tap;
            if (g > 0 && g < n_cells) {                 // bin 0 is never written (RadarCPU.cpp:424)
                const float v = (float)((double)r.strength * (double)(w ? w[tap] : 1.0f));
                if (v > 0.0f && v < __builtin_inff())   // (false for NaN)
                    atomicMax(&s_key[g], ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)(0xFFFFFFFFu - k));
            }
        }
        k += dk; tap += dt;
        if (tap >= (uint32_t)W) { tap -= (uint32_t)W; k++; }
    }
    __syncthreads();
    for (int g = threadIdx.x; g < n_cells; g += 256) {
        const unsigned long long key = s_key[g];
        uint32_t info = kNoLabel, face = kNoLabel;
        if (key) { const EchoSrc r = list[0xFFFFFFFFu - (uint32_t)key]; info = r.info; face = r.face; }
        label_cols[(size_t)seg * n_cells + g] = info;
        face_cols[(size_t)seg * n_cells + g] = face;
    }
}

// grid n_seg, block 256.  dst rows may start at any 4-byte boundary (the caller's buffer)
__global__ __launch_bounds__(256) void k_echo_export(const EchoSrc* __restrict__ lists, const uint32_t* __restrict__ counts, const size_t cap,
                                                     rr_echo_src* __restrict__ dst, const size_t stride, uint32_t* __restrict__ dst_counts)
{
    const int seg = blockIdx.x;
    const uint32_t n = counts[seg];
    const size_t m = min(min((size_t)n, cap), stride);
    for (size_t i = threadIdx.x; i < m; i += 256) {
        const EchoSrc r = lists[(size_t)seg * cap + i];
        rr_echo_src o; o.cell = r.cell; o.strength = r.strength; o.face = r.face; o.info = r.info;
        dst[(size_t)seg * stride + i] = o;
    }
    if (threadIdx.x == 0) dst_counts[seg] = n;
}

void launch_echo_gather(const Params& P, int pass, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop)
{
    launch_k(k_echo_gather, dim3(P.n_seg), dim3(256), 0, s, ev_start, ev_stop, P, pass);
}

void launch_label(const EchoSrc* lists, const uint32_t* counts, size_t stride, int n_seg, int n_cells, int W, int mode, const float* w,
                  uint32_t* label_cols, uint32_t* face_cols, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop)
{
    launch_k(k_label, dim3(n_seg), dim3(256), (size_t)n_cells * sizeof(unsigned long long), s, ev_start, ev_stop, lists, counts, stride, n_cells,
             W, mode, w, label_cols, face_cols);
}

void launch_echo_export(const EchoSrc* lists, const uint32_t* counts, size_t cap, int n_seg, rr_echo_src* dst, size_t stride, uint32_t* dst_counts,
                        hipStream_t s)
{
    hipLaunchKernelGGL(k_echo_export, dim3(n_seg), dim3(256), 0, s, lists, counts, cap, dst, stride, dst_counts);
}

}  // namespace rr
