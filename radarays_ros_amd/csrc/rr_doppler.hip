// rr_doppler.hip -- Doppler (rr_simulate_batch_doppler_device; the definition of an echo's range rate and of its shifted cell is in
// include/radarays_mi355.h).  The rate of an echo is a sum along the chain of waves that led to it; the chain's kernels keep neither a
// wave's parent nor its map-frame ray past two passes.  These kernels run beside a frame chain whose own kernels do not change (the
// chain is the provenance chain: k_echo_gather has left the lane's echo lists, which give the order and the strengths):
//
//   k_rate_gather   behind the k_shade launch of EVERY pass, one 256-thread workgroup per segment, walking the pass' live list in
//                   position order like k_wave_gather.  Per wave it forms the map-frame ray exactly as k_wave_gather's RR_WAVES_MAP_FRAME
//                   records do, reads its parent's state (position slot >> 1 of the previous pass) and keeps its own: ONE f32 running
//                   sum  A_k = -v_s.u_0 + sum_{i<k} v_i.(u_i - u_{i+1})  beside the v_k and u_k its children will need -- 32 bytes per wave,
//                   ping-pong by pass parity, so no echo walks its parents.  Per echo of the wave (k_wave_gather's echo index: echoes of
//                   earlier passes + the stable prefix over slot order) it writes (v_r, signal_dist) into the lane's rate list.
//   k_doppler_shift once behind the chain's k_column, over the lane's echo lists: r' = signal_dist + gain * v_r, cell', and the
//                   outputs: the caller's v_r / cell' rows (the first `stride` of a longer list), the true counts, and the lane's
//                   shifted (cell', strength) list, which launch_column then replays as a list-only stream (rr_debug_column's form).
//   k_vel_winner    the label rule (k_label's 64-bit LDS keys: largest single term, ties to the earlier echo) on the shifted cells; the
//                   winner's v_r per bin, NaN where nobody reaches the bin.
//
// All f32, built with -ffp-contract=off like the rest: the sums are in the order the header states.  No kernel uses scratch;
// k_rate_gather 32 B of static LDS (the scan's), k_vel_winner dynamic LDS only (8 B per cell).  Vector stores only.
#include "../../include/radarays_mi355.h"
#include "rr_device.h"
#include "rr_launch.h"

namespace rr {

// RadarCPU.cpp:410-411 as signal_cell (rr_kernels.hip) forms it, without the division by the resolution
__device__ inline float signal_dist_of(double time)
{
    const float half_time = (float)(time / 2.0);
    return (float)(0.3 * (double)half_time);
}

// grid n_seg, block 256
__global__ __launch_bounds__(256) void k_rate_gather(const Params P, const int pass, const DopArgs D)
{
    __shared__ int lds[8];
    const int seg = blockIdx.x;
    const int cur = pass & 1;
    const int count = pass == 0 ? P.n_beam : (int)P.count[cur][seg];
    // a wave owns two slots; the last pass' odd ones are written only with record_multi_path
    const bool odd = !(pass == P.n_passes - 1 && !P.record_multi_path);
    const size_t base1 = (size_t)seg * P.cap, base2 = 2 * base1;
    uint32_t n_echo = pass == 0 ? 0u : D.count[seg];
    Quat q_am; V3 t_am;
    azimuth_frame<false>(P, nullptr, seg, q_am, t_am);
    const float4 vs4 = D.in[seg / P.n_loc];
    const V3 v_s = { vs4.x, vs4.y, vs4.z };
    const size_t par_stride = (size_t)P.n_seg * P.cap * 2;       // float4 per parity
    float4* mine = D.wstate + (size_t)cur * par_stride + base1 * 2;
    const float4* theirs = D.wstate + (size_t)(cur ^ 1) * par_stride + base1 * 2;
    float2* rate = D.rate + (size_t)seg * P.prov_cap;

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
        if (live) {
            V3 o = { 0.0f, 0.0f, 0.0f }, d;
            double time = 0.0;        // RadarCPU.cpp:112
            float4 pa = make_float4(0.0f, 0.0f, 0.0f, 0.0f), pb = pa;
            if (pass == 0) {
                const float4 bm = P.beams[j];
                d = { bm.x, bm.y, bm.z };
            } else {
                const uint32_t slot = P.idx[cur][base1 + j];
                const size_t w = base2 + slot;
                const float4 A = P.waves[cur].A[w], B = P.waves[cur].B[w];
                o = { A.x, A.y, A.z };
                d = { A.w, B.x, B.y };
                time = P.waves[cur].C[w].y;
                pa = theirs[2 * (size_t)(slot >> 1)]; pb = theirs[2 * (size_t)(slot >> 1) + 1];
            }
            // the map-frame ray: the expressions k_trace sets its ray up with (k_wave_gather under RR_WAVES_MAP_FRAME)
            const V3 om = pass == 0 ? t_am : v_add(q_rot(q_am, o), t_am);
            const V3 u = q_rot(q_am, d);
            float acc;
            if (pass == 0) acc = -v_dot(v_s, u);
            else {
                const V3 vp = { pa.x, pa.y, pa.z }, up = { pb.x, pb.y, pb.z };
                acc = pa.w + v_dot(vp, v_sub(up, u));
            }
            const uint2 h = P.hit[base1 + j];
            const float range = __uint_as_float(h.x);
            V3 v = { 0.0f, 0.0f, 0.0f };
            if (range >= 0.0f) {
                const float4* tp = reinterpret_cast<const float4*>(P.tris + h.y);
                const uint32_t obj = __float_as_uint(tp[1].w) & 0xFFFFFFu;
                const V3 p = v_add(om, v_scale(u, range));
                if (obj < D.n_objects) {
                    const float4 tv = D.in[64 + 2 * (size_t)obj], tw = D.in[64 + 2 * (size_t)obj + 1];
                    const V3 V = { tv.x, tv.y, tv.z }, Om = { tw.x, tw.y, tw.z };
                    v = v_add(V, v_cross(Om, p));
                }
                if (g0 | g1) {
                    const float dl = acc + v_dot(v, u);
                    const double t_hit = time + (double)range / 0.3;          // wave.move(range), radar_types.h:108-113
                    uint32_t pos = n_echo + (uint32_t)pre;
                    if (g0) {
                        const float time_back = (float)(t_hit * 2.0);           // RadarCPU.cpp:319-323
                        if (pos < (uint32_t)P.prov_cap) rate[pos] = make_float2(dl, signal_dist_of((double)time_back));
                        pos++;
                    }
                    if (g1) {                                                   // RadarCPU.cpp:325-360: straight back to the sensor
                        const V3 io = v_add(o, v_scale(d, range));
                        const float dist = sqrtf(io.x * io.x + io.y * io.y + io.z * io.z);
                        const V3 e = v_normalize(v_sub(p, t_am));
                        const float vr = 0.5f * (dl + v_dot(v_sub(v, v_s), e));
                        if (pos < (uint32_t)P.prov_cap) rate[pos] = make_float2(vr, signal_dist_of(t_hit + (double)dist / 0.3));
                    }
                }
            }
            if (pass < P.n_passes - 1) {      // (the last pass has no children)
                mine[2 * (size_t)j] = make_float4(v.x, v.y, v.z, acc);
                mine[2 * (size_t)j + 1] = make_float4(u.x, u.y, u.z, 0.0f);
            }
        }
        n_echo += (uint32_t)tot;
    }
    __syncthreads();        // every thread has read the count (a pass with no wave runs no scan, so no barrier)
    if (threadIdx.x == 0) D.count[seg] = n_echo;
}

// the shifted cell of one echo (-1: dropped)
__device__ inline int32_t shifted_cell(float signal_dist, float gain, float vr, double resolution)
{
    const float r = signal_dist + gain * vr;
    const double q = (double)r / resolution;
    return (q >= 0.0 && q < 2147483648.0) ? (int32_t)q : -1;       // (false for NaN)
}

// grid n_seg, block 256
__global__ __launch_bounds__(256) void k_doppler_shift(const Params P, const DopArgs D)
{
    const int seg = blockIdx.x;
    const uint32_t n = D.count[seg];
    const uint32_t m = min(n, (uint32_t)P.prov_cap);
    const EchoSrc* list = P.prov + (size_t)seg * P.prov_cap;
    const float2* rate = D.rate + (size_t)seg * P.prov_cap;
    SigRec* out = D.shifted + (size_t)seg * P.prov_cap;
    for (uint32_t i = threadIdx.x; i < m; i += 256) {
        const float2 r = rate[i];
        SigRec s;
        s.cell = shifted_cell(r.y, D.gain, r.x, P.resolution);
        s.strength = list[i].strength;
        out[i] = s;
        if ((size_t)i < D.stride) {
            if (D.echo_vel) D.echo_vel[(size_t)seg * D.stride + i] = r.x;
            if (D.echo_cells) D.echo_cells[(size_t)seg * D.stride + i] = s.cell;
        }
    }
    __syncthreads();        // every thread has read the count
    if (threadIdx.x == 0) {
        D.count[seg] = m;           // what k_column and k_vel_winner read: the length of the lane's list
        if (D.echo_counts) D.echo_counts[seg] = n;
    }
}

// grid n_seg, block 256, dynamic LDS 8 B x n_cells.  w null: no denoiser (W = 1, mode = 0, weight 1).  k_label's rule on the shifted list
__global__ __launch_bounds__(256) void k_vel_winner(const SigRec* __restrict__ lists, const float2* __restrict__ rates, const uint32_t* __restrict__ counts,
                                                    const size_t stride, const int n_cells, const int W, const int mode, const float* __restrict__ w,
                                                    float* __restrict__ vel_cols)
{
    extern __shared__ unsigned long long s_key[];       // [n_cells] 0: nobody reached the bin
    const int seg = blockIdx.x;
    const SigRec* list = lists + (size_t)seg * stride;
    const uint32_t n = (uint32_t)min((size_t)counts[seg], stride);
    for (int g = threadIdx.x; g < n_cells; g += 256) s_key[g] = 0ull;
    __syncthreads();
    const uint32_t dk = 256u / (uint32_t)W, dt = 256u % (uint32_t)W;
    uint32_t k = threadIdx.x / (uint32_t)W, tap = threadIdx.x % (uint32_t)W;
    while (k < n) {
        const SigRec r = list[k];
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
        float v = __uint_as_float(0x7FC00000u);
        if (key) v = rates[(size_t)seg * stride + (0xFFFFFFFFu - (uint32_t)key)].x;
        vel_cols[(size_t)seg * n_cells + g] = v;
    }
}

void launch_rate_gather(const Params& P, int pass, const DopArgs& D, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop)
{
    launch_k(k_rate_gather, dim3(P.n_seg), dim3(256), 0, s, ev_start, ev_stop, P, pass, D);
}

void launch_doppler_shift(const Params& P, const DopArgs& D, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop)
{
    launch_k(k_doppler_shift, dim3(P.n_seg), dim3(256), 0, s, ev_start, ev_stop, P, D);
}

void launch_vel_winner(const Params& P, const DopArgs& D, hipStream_t s, hipEvent_t ev_start, hipEvent_t ev_stop)
{
    const bool den = P.signal_denoising > 0;
    launch_k(k_vel_winner, dim3(P.n_seg), dim3(256), (size_t)P.n_cells * sizeof(unsigned long long), s, ev_start, ev_stop,
             (const SigRec*)D.shifted, (const float2*)D.rate, (const uint32_t*)D.count, (size_t)P.prov_cap, P.n_cells, den ? P.smear_w : 1,
             den ? P.smear_mode : 0, den ? P.smear : (const float*)nullptr, D.vel_cols);
}

}  // namespace rr
