// rr_stage.h -- Scratch: a call's rooms in a pool of anonymous device buffers that only grow.  Stage: the round trip of a host form over such
// a pool.  Its inputs go up into fresh room, a device form runs on that room, its outputs come home.
//
// The pools: rr_ctx::stage for the host forms on c->stream, Lane::stage for the host forms of rr_side.hip (lanes overlap in time), and for
// the device forms one pool per stream they have been called on (rr_ctx::scratch_of).  Request i of a call takes slot i, so a pointer handed
// out earlier in the call never moves, and every pointer is hipMalloc's own (16-byte aligned: the device forms refuse unaligned tables,
// states and records, and kernels read scratch with 16-byte loads).  A slot that grows is freed first, and an earlier call's kernels may
// still read it: the stream is drained before that, once per call at the most.  A host form drains its stream itself before it opens its Stage.
//
// The rule for outputs, said once: a HELD output goes through a host vector and reaches the caller in commit(), after every copy has
// landed and the gate has passed -- a call that fails at any step has written nothing through it.  A DIRECT output is copied straight
// into the caller's buffer once the gate has passed: bulk images (rr_detect, rr_polar_to_cartesian, rr_polar_to_cartesian_sweep, what
// the rr_simulate_batch_* forms hand out beside their records), which gain no second host copy.  The chunked forms bring each chunk's
// surfaces home themselves, a chunk at a time.
#pragma once
#include "rr_ctx.h"
#include "rr_rows.h"
#include <algorithm>

namespace rr {

struct Scratch {
    StagePool& pool; hipStream_t s; size_t used = 0; bool drained;
    Scratch(StagePool& pool_, hipStream_t s_, bool drained_ = false) : pool(pool_), s(s_), drained(drained_) {}

    // room for n elements -> d.  n = 0 takes its slot all the same (a form keeps its slot order with and without its optional rooms), allocates
    // nothing and gives null
    template <class T> hipError_t room(size_t n, T*& d)
    {
        d = nullptr;
        if (used == pool.size()) pool.emplace_back();
        DevBuf<uint4>& b = pool[used++];
        const size_t words = (n * sizeof(T) + sizeof(uint4) - 1) / sizeof(uint4);
        if (words > b.n) {
            hipError_t e = drained ? hipSuccess : hipStreamSynchronize(s);
            drained = true;
            if (e == hipSuccess) e = b.ensure(words);
            if (e != hipSuccess) return e;
        }
        if (words) d = reinterpret_cast<T*>(b.p);
        return hipSuccess;
    }
};

struct Stage : Scratch {
    struct Out { void* dst; const void* d_src; size_t bytes, elem, n_rows, d_stride, stride; const void* counts; bool held; std::vector<uint8_t> h; };
    rr_ctx* c;
    std::vector<Out> outs;
    Stage(rr_ctx* c_, StagePool& pool_, hipStream_t s_) : Scratch(pool_, s_, true), c(c_) {}      // (drained by the caller)

    // room for n elements -> d, never null: the device forms refuse a null buffer, an empty one too
    template <class T> hipError_t room(size_t n, T*& d) { return Scratch::room(std::max<size_t>(n, 1), d); }
    // a host array the caller gave (else d = null and that is all) into fresh room -> d; again(): the next chunk into the same room
    template <class T> hipError_t up(const T* h, size_t n, T*& d)
    {
        d = nullptr;
        if (!h) return hipSuccess;
        const hipError_t e = room(n, d);
        return e == hipSuccess ? again(d, h, n) : e;
    }
    template <class T> hipError_t again(T* d, const T* h, size_t n) { return n ? hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, s) : hipSuccess; }
    // ... n_rows rows of `stride` elements, of row a its first min(counts[a], stride): nothing beyond them moves
    template <class T> hipError_t up_rows(const T* h, size_t n_rows, size_t stride, const uint32_t* counts, T*& d)
    {
        hipError_t e = room(n_rows * stride, d);
        for (size_t a = 0; a < n_rows && e == hipSuccess; a++) e = again(d + a * stride, h + a * stride, std::min<size_t>(counts[a], stride));
        return e;
    }

    // An output the caller asked for (dst non-null; else nothing): n elements at d_src, held or direct
    template <class T> void out(T* dst, const T* d_src, size_t n, bool held = true) { out_rows(dst, d_src, 1, n, n, nullptr, held); }
    // ... as n_rows rows of d_stride elements for the caller's rows of `stride` elements, of which row a receives its first
    // min(counts[a], d_stride) (scatter_rows).  counts: the caller's buffer of another held output (a uint32 per row), or a host array
    template <class T> void out_rows(T* dst, const T* d_src, size_t n_rows, size_t d_stride, size_t stride, const void* counts, bool held = true)
    {
        if (dst) outs.push_back(Out{ dst, d_src, n_rows * d_stride * sizeof(T), sizeof(T), n_rows, d_stride, stride, counts, held, {} });
    }
    // ... held, from fresh room -> d (dst null: d = null)
    template <class T> hipError_t hold(T* dst, size_t n, T*& d) { return hold_rows(dst, 1, n, n, nullptr, d); }
    template <class T> hipError_t hold_rows(T* dst, size_t n_rows, size_t d_stride, size_t stride, const void* counts, T*& d)
    {
        d = nullptr;
        if (!dst) return hipSuccess;
        const hipError_t e = room(n_rows * d_stride, d);
        out_rows(dst, d, n_rows, d_stride, stride, counts);
        return e;
    }

    // The way out: the launches' error, the held copies behind them on s, the lane handed back behind those (rr_side.hip), the stream
    // drained, the gate (the frame's error bits, where a frame was simulated) -- and only then the caller's buffers
    template <class Gate> int commit(Gate gate, Lane* lane = nullptr)
    {
        RR_HIP(c, hipGetLastError());
        for (Out& o : outs)
            if (o.held) { o.h.resize(o.bytes); if (o.bytes) RR_HIP(c, hipMemcpyAsync(o.h.data(), o.d_src, o.bytes, hipMemcpyDeviceToHost, s)); }
        if (lane) RR_HIP(c, give_lane(*lane, s));
        RR_HIP(c, hipStreamSynchronize(s));
        const int rc = gate(); if (rc) return rc;
        bool direct = false;
        for (const Out& o : outs)
            if (!o.held && o.bytes) { direct = true; RR_HIP(c, hipMemcpyAsync(o.dst, o.d_src, o.bytes, hipMemcpyDeviceToHost, s)); }
        if (direct) RR_HIP(c, hipStreamSynchronize(s));
        for (const Out& o : outs) {
            if (!o.held) continue;
            if (!o.counts) { if (o.bytes) std::memcpy(o.dst, o.h.data(), o.bytes); continue; }
            const auto n = std::find_if(outs.begin(), outs.end(), [&](const Out& x) { return x.held && x.dst == o.counts; });
            scatter_rows(o.dst, o.stride, o.h.data(), o.d_stride, o.elem, o.n_rows,
                         reinterpret_cast<const uint32_t*>(n != outs.end() ? n->h.data() : o.counts));
        }
        return 0;
    }
    int commit() { return commit([] { return 0; }); }
};

// a host form on c->stream opens its stage `st`: the stream drained first (see the top of this file)
#define RR_STAGE(c, st) RR_HIP(c, hipStreamSynchronize((c)->stream)); Stage st((c), (c)->stage, (c)->stream)

}  // namespace rr
