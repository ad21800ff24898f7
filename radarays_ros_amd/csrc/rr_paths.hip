// rr_paths.hip -- wave paths (rr_simulate_batch_paths_device; the definition of a wave record is in include/radarays_mi355.h).
// A wave's origin, direction, energy, time and medium live in the ping-pong queue waves[pass & 1]; k_shade overwrites that queue two
// passes later, and the next pass' k_trace overwrites hit[].  This kernel keeps them, beside a frame chain whose own kernels do not change:
//
//   k_wave_gather  behind the k_shade launch of EVERY pass (the last included), one 256-thread workgroup per segment: walks the pass'
//                  live list in position order, j = 0 .. count in sweeps of 256, and writes one 64-byte record per wave straight into the
//                  caller's row at (waves of earlier passes + j): the wave as the queue holds it (slot idx[cur][j]; pass 0: beam j), its
//                  hit[seg][j] with the face / object of the triangle, its parent (start of the previous pass + slot >> 1), its branch
//                  (1 + (slot & 1)) and the index of its first echo: echoes of earlier passes + the stable exclusive prefix of
//                  cell >= 0 over slot order (block_excl_scan over the two slots of every position: k_echo_gather's count).  The last
//                  pass' odd slots exist only with record_multi_path and are read only then (k_column's sl_sh rule).  The walk follows
//                  idx[cur], not the last pass' shade order: k_shade<., LAST> never reads the record of a wave inside a material, but
//                  the queue still holds it and every output stays indexed by the wave's own position.
//                  Per-segment state {waves so far, start of the previous pass, echoes so far} in the lane's buffer: pass 0 writes it,
//                  later passes advance it -- no memset in the chain.  Reads count, idx, waves, hit, tris, sigtmp; writes only the
//                  caller's rows, the counts and the state.
//
// A latency / scatter-read kernel like k_echo_gather: per position one 4-B slot load, then three dependent 16-B loads of the wave, an
// 8-B hit load and two 16-B triangle words behind it.  A lane's record is four 16-B stores at a 64-B pitch: the four store
// instructions of a wave cover 4 KB of the row contiguously between them.  No scratch; 32 B of static LDS (the scan's) and the barrier.
#include "../../include/radarays_mi355.h"
#include "rr_device.h"
#include "rr_launch.h"
#include <cstddef>

namespace rr {

static_assert(sizeof(rr_wave_rec) == 64 && offsetof(rr_wave_rec, d) == 16 && offsetof(rr_wave_rec, energy) == 32 && offsetof(rr_wave_rec, info) == 48,
              "a record is written as four 16-byte words");
static_assert(kWavePasses == RR_WAVES_MAX_PASSES, "the header states the kernel's constant");

// grid n_seg, block 256
__global__ __launch_bounds__(256) void k_wave_gather(const Params P, const int pass, const WaveOut W)
{
    __shared__ int lds[8];
    const int seg = blockIdx.x;
    const int cur = pass & 1;
    const int count = pass == 0 ? P.n_beam : (int)P.count[cur][seg];
    // a wave owns two slots; the last pass' odd ones are written only with record_multi_path
    const bool odd = !(pass == P.n_passes - 1 && !P.record_multi_path);
    const size_t base1 = (size_t)seg * P.cap, base2 = 2 * base1;
    uint4 st = make_uint4(0u, 0u, 0u, 0u);
    if (pass > 0) st = W.state[seg];
    const uint32_t first = st.x, prev = st.y;
    uint32_t n_echo = st.z;
    const bool map = (W.flags & RR_WAVES_MAP_FRAME) != 0;
    Quat q_am = { 0.0f, 0.0f, 0.0f, 1.0f }; V3 t_am = { 0.0f, 0.0f, 0.0f };
    if (map) azimuth_frame<false>(P, nullptr, seg, q_am, t_am);
    float4* row = W.recs ? W.recs + (size_t)seg * W.stride * 4 : nullptr;

    for (int b = 0; b < count; b += 256) {
        const int j = b + (int)threadIdx.x;
        const bool live = j < count;
        int g0 = 0, g1 = 0;
        if (live) {
            g0 = P.sigtmp[base2 + 2 * (size_t)j].cell >= 0 ? 1 : 0;
            if (odd) g1 = P.sigtmp[base2 + 2 * (size_t)j + 1].cell >= 0 ? 1 : 0;
        }
        int tot;
        const int pre = block_excl_scan(g0 + g1, tot, lds);
        const size_t at = (size_t)first + (size_t)j;
        if (live && row && at < W.stride) {
            V3 o = { 0.0f, 0.0f, 0.0f }, d;
            double energy = 1.0, time = 0.0;        // RadarCPU.cpp:107,112
            uint32_t mat = 0, branch = 0;           // RadarCPU.cpp:111
            int32_t parent = -1;
            if (pass == 0) {
                const float4 bm = P.beams[j];
                d = { bm.x, bm.y, bm.z };
            } else {
                const uint32_t slot = P.idx[cur][base1 + j];
                const size_t w = base2 + slot;
                const float4 A = P.waves[cur].A[w], B = P.waves[cur].B[w];
                const double2 C = P.waves[cur].C[w];
                o = { A.x, A.y, A.z };
                d = { A.w, B.x, B.y };
                mat = __float_as_uint(B.z);
                energy = C.x; time = C.y;
                parent = (int32_t)(prev + (slot >> 1));
                branch = 1u + (slot & 1u);
            }
            const uint2 h = P.hit[base1 + j];
            uint32_t face = kNoLabel, obj = 0xFFFFFFu;
            if (__uint_as_float(h.x) >= 0.0f) {
                const float4* tp = reinterpret_cast<const float4*>(P.tris + h.y);
                face = __float_as_uint(tp[0].w);
                obj = __float_as_uint(tp[1].w) & 0xFFFFFFu;
            }
            if (map) {      // the expressions k_trace sets its ray up with (pass 0: every ray starts in t_am)
                o = pass == 0 ? t_am : v_add(q_rot(q_am, o), t_am);
                d = q_rot(q_am, d);
            }
            const uint32_t info = obj | ((uint32_t)pass << 24) | (branch << 28) | ((uint32_t)g0 << 30) | ((uint32_t)g1 << 31);
            const int32_t echo = (g0 | g1) ? (int32_t)(n_echo + (uint32_t)pre) : -1;
            float4* r = row + at * 4;
            r[0] = make_float4(o.x, o.y, o.z, __uint_as_float(h.x));
            r[1] = make_float4(d.x, d.y, d.z, __uint_as_float(face));
            *reinterpret_cast<double2*>(r + 2) = make_double2(energy, time);
            *reinterpret_cast<uint4*>(r + 3) = make_uint4(info, (uint32_t)parent, mat, (uint32_t)echo);
        }
        n_echo += (uint32_t)tot;
    }
    __syncthreads();        // every thread has read the state (a pass with no wave runs no scan, so no barrier)
    if (threadIdx.x == 0) {
        W.state[seg] = make_uint4(first + (uint32_t)count, first, n_echo, 0u);
        if (W.counts) W.counts[seg] = first + (uint32_t)count;
    }
    if (W.pass_counts) {
        uint32_t* pc = W.pass_counts + (size_t)seg * kWavePasses;
        if (pass == 0) { if (threadIdx.x < kWavePasses) pc[threadIdx.x] = threadIdx.x == 0 ? (uint32_t)count : 0u; }      // the passes that never run stay 0
        else if (threadIdx.x == 0 && pass < kWavePasses) pc[pass] = (uint32_t)count;
    }
}

void launch_wave_gather(const Params& P, int pass, const WaveOut& W, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop)
{
    launch_k(k_wave_gather, dim3(P.n_seg), dim3(256), 0, s, ev_start, ev_stop, P, pass, W);
}

}  // namespace rr
