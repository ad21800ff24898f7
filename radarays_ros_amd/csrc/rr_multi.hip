// rr_multi.hip -- multi-GPU fan-out BEHIND the C ABI (SURVEY.md §8b "Threading": one backend object per process,
// radar_simulator.cpp:145-176; §8e: azimuth columns are independent, RadarCPU.cpp:155).
//
// One process, one rr_ctx per device, mesh / parameters replicated, device i renders the contiguous azimuth block
// rr_partition(n_angles, n, i) of every frame of a call in ONE set of launches on its own stream; ONE RCCL
// collective per call GATHERS the blocks on device 0 (the root) -- one ncclGroup of send / recv pairs along
// rr_multi_plan: one piece per device for equal blocks, one per device and frame for ragged ones; nobody but the
// root receives anything -- then the root transposes into mono8 images and copies them to the caller's host buffer.
// Calls are PIPELINED (round 4): rr_multi_simulate_batch_async enqueues a batch on one of RR_MULTI_SLOTS (4) slots --
// own stream + block buffer per device, own receive / image buffers on the root -- and returns; rr_multi_wait is the
// consumer's fence.  The render of batch k+1 overlaps the collective, transpose and D2H copy of batch k, like the
// slots of dist.py's step loop.  Per-batch error bits travel to page-locked host words (rr_peek_error_bits_async), so
// no call drains a device unless something failed.
// RCCL is loaded at run time (librccl.so.1): the library itself has no link-time dependency on it and
// rr_create_multi() fails with a clear message where it is missing.  Built on the public entry points of
// radarays_mi355.h only.
#include "../../include/radarays_mi355.h"
#include "rr_devbuf.h"
#include "rr_hostprof.h"

#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

// the part of the RCCL API this file uses (rccl.h: same prototypes as NCCL 2)
typedef struct ncclComm* ncclComm_t;
typedef int ncclResult_t;
typedef int ncclDataType_t;
constexpr ncclDataType_t kNcclUint8 = 1;   // ncclUint8 / ncclChar family: ncclInt8 = 0, ncclUint8 = 1
#define RR_SYM(f) f = (decltype(f))dlsym(lib, "nccl" #f); if (!f) { err = "rr_create_multi: librccl lacks nccl" #f; return false; }
struct Rccl {
    void* lib = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*GetVersion)(int*) = nullptr;
    int version = 0;                       // ncclGetVersion's code (2.27.7 -> 22707), 0: the library does not say
    bool load(std::string& err) {
        if (lib) return true;
        for (const char* n : { "librccl.so.1", "librccl.so" }) { lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (lib) break; }
        if (!lib) { err = "rr_create_multi: librccl.so.1 not found (RCCL is needed for more than one device)"; return false; }
        RR_SYM(CommInitAll) RR_SYM(CommDestroy) RR_SYM(Send) RR_SYM(Recv) RR_SYM(GroupStart) RR_SYM(GroupEnd) RR_SYM(GetErrorString)
        // The prototypes above are declared BY HAND (the library is loaded at run time, rccl.h is not included): they are those of
        // the NCCL 2 API from 2.7 on (ncclSend / ncclRecv; rccl.h of ROCm 7.2: 2.27.7, checked against the header by
        // tests/test_abi.py).  A library that reports a version outside [2.7, 3.0) is refused instead of being called
        // through signatures nobody has compared; one that reports none is accepted and left to the self-test below
        GetVersion = (decltype(GetVersion))dlsym(lib, "ncclGetVersion");
        if (GetVersion && GetVersion(&version) == 0) {
            const bool ok = (version >= 20900 && version < 30000) || (version >= 2700 && version < 2900);    // (2.9 changed the code's format)
            if (!ok) {
                err = "rr_create_multi: librccl reports NCCL version code " + std::to_string(version) +
                      ", outside the range this library's hand-declared prototypes were checked for (2.7 .. 2.x)";
                return false;
            }
        } else version = 0;
        return true;
    }
};
#undef RR_SYM
Rccl g_rccl;
std::string g_multi_create_error;

}  // namespace

// one batch in flight: its own stream and block buffer on every device, the root's receive / image buffers, the host
// words the devices' error bits arrive in
struct MultiSlot {
    std::vector<hipStream_t> streams;     // per device
    std::vector<rr::DevBuf<uint8_t>> block;// per device: [n_frames][n_loc_i][n_cells]
    std::vector<hipEvent_t> ev_block;     // per device: block rendered (loopback: the root's copies wait for it)
    rr::DevBuf<uint8_t> gathered;         // root: what the collective delivers
    rr::DevBuf<uint8_t> d_imgs;           // root: [n_frames][n_cells][n_angles]
    hipEvent_t ev_done = nullptr;         // root: images in the caller's buffer
    uint32_t* h_bits = nullptr;           // page-locked [n_devices]: rr_peek_error_bits_async
    const void* dst = nullptr;            // the caller's buffer of the batch in flight
    bool pending = false;
    int failed = 0;                       // != 0: this batch was in flight when another one's error drained the object -- its
                                          // images are not to be trusted (error bits are per frame lane, not per batch, and a
                                          // drain reads and clears them all); reported by the wait for its buffer / the next use of the slot
    bool owns_streams = true;             // one device: twice as many records as streams (see create_slots)
};

// One enqueue thread per device: a call's launches for device i (a dozen kernels, an event, a copy: 60-100 us of host time)
// are issued by worker i while the others issue theirs -- from ONE thread the host side of a call grows with the number
// of devices (measured in loopback, config 2, 8 entries: 450 us per 8-frame call = a cap of 17.6k images/s whatever the GPUs
// do).  A context is used by one thread at a time (the header's rule): worker i is the only one that touches context i
// while a call renders; the caller's thread takes over (collective, root) only after every worker has reported back.
struct MultiWorker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::function<void()> job;
    bool has_job = false, done = false, quit = false;
    ~MultiWorker() { { std::lock_guard<std::mutex> lk(mu); quit = true; } cv.notify_all(); if (th.joinable()) th.join(); }
};

struct rr_multi {
    std::vector<std::unique_ptr<MultiWorker>> workers;     // empty: the caller's thread issues everything (the default; RR_MULTI_THREADS=1 starts them)
    std::vector<int> devices;
    std::vector<rr_ctx*> ctx;
    std::vector<ncclComm_t> comms;
    std::vector<MultiSlot> slots;         // batches in flight
    size_t next_slot = 0;
    rr_config cfg;
    bool have_cfg = false;
    // the switches, read once by rr_create_multi
    bool loopback = false;                // RR_MULTI_LOOPBACK (see rr_create_multi)
    int n_streams = 4;                    // RR_MULTI_SLOTS: streams per device = batches in flight (see create_slots)
    bool self_rccl = false;               // RR_MULTI_SELF_RCCL=1 with ONE device: its block travels to itself through RCCL (test switch)
    bool self_rccl_frames = false;        // ... =2: frame by frame (the ragged plan's many pieces in one group)
    bool threads = false;                 // RR_MULTI_THREADS with several devices: one MultiWorker each
    std::string err;
};

namespace {

int env_int(const char* value, int unset) { return value ? atoi(value) : unset; }
int mfail(rr_multi* m, int code, const std::string& msg) { if (m) m->err = msg; else g_multi_create_error = msg; return code; }

// "device N: what": `what` is entry i's context's own message unless the caller brings one (a HIP error's text)
std::string dev_err(const rr_multi* m, size_t i, const std::string& what = std::string()) { return "device " + std::to_string(m->devices[i]) + ": " + (what.empty() ? std::string(rr_last_error(m->ctx[i])) : what); }

// `call(context, i)` on every device entry in turn; the first that fails ends it, and its context's message is kept
template <typename PerDevice>
int on_each(rr_multi* m, PerDevice call)
{
    if (!m) return -1;
    for (size_t i = 0; i < m->ctx.size(); i++) { const int rc = call(m->ctx[i], i); if (rc) return mfail(m, rc, dev_err(m, i)); }
    return 0;
}

// a tree is made ONCE, on device 0 (a build: 1.9 s of host time at 10M triangles); the finished tree then goes from
// device to device (rr_copy_mesh: xGMI), rest geometry and poses with it
template <typename Build>
int replicate_tree(rr_multi* m, Build build_on_root)
{
    return on_each(m, [&](rr_ctx* c, size_t i) { return i == 0 ? build_on_root(c) : rr_copy_mesh(c, m->ctx[0]); });
}

// ---- enqueue threads ------------------------------------------------------------------------------------------
void worker_loop(MultiWorker* w, int dev)
{
    (void)hipSetDevice(dev);
    std::unique_lock<std::mutex> lk(w->mu);
    for (;;) {
        w->cv.wait(lk, [w] { return w->has_job || w->quit; });
        if (w->quit) return;
        w->has_job = false;
        lk.unlock();
        w->job();
        lk.lock();
        w->done = true;
        w->cv.notify_all();
    }
}

void post(MultiWorker* w, std::function<void()> job)
{
    { std::lock_guard<std::mutex> lk(w->mu); w->job = std::move(job); w->done = false; w->has_job = true; }
    w->cv.notify_all();
}

void collect(MultiWorker* w) { std::unique_lock<std::mutex> lk(w->mu); w->cv.wait(lk, [w] { return w->done; }); }

void start_workers(rr_multi* m)
{
    for (const int dev : m->devices) {
        m->workers.emplace_back(new MultiWorker());
        MultiWorker* w = m->workers.back().get();
        try { w->th = std::thread(worker_loop, w, dev); }
        catch (...) { m->workers.clear(); return; }            // no thread to be had: the caller's thread does the work
    }
}

// ---- the one RCCL group -----------------------------------------------------------------------------------------
struct Piece { int dev; const uint8_t* src; uint8_t* dst; size_t bytes; };       // `bytes` at `src` on entry `dev` -> `dst` on the root
struct GroupError { hipError_t hip = hipSuccess; ncclResult_t nccl = 0; };

// ONE group of send / recv pairs, every piece from its device to the root, each on its device's stream of slot S.  One
// thread drives every device: the current device follows the communicator a call is made on.  A failure inside the
// group still closes the group; what comes back is the first thing that went wrong.
GroupError send_to_root(rr_multi* m, MultiSlot& S, const std::vector<Piece>& pieces)
{
    GroupError r;
    const ncclResult_t opened = g_rccl.GroupStart();
    ncclResult_t posted = 0;
    for (const Piece& p : pieces) {
        if (opened != 0 || posted != 0 || r.hip != hipSuccess) break;
        const size_t d = (size_t)p.dev;
        r.hip = hipSetDevice(m->devices[d]);
        if (r.hip == hipSuccess) posted = g_rccl.Send(p.src, p.bytes, kNcclUint8, 0, m->comms[d], S.streams[d]);
        if (r.hip == hipSuccess && posted == 0) r.hip = hipSetDevice(m->devices[0]);
        if (r.hip == hipSuccess && posted == 0) posted = g_rccl.Recv(p.dst, p.bytes, kNcclUint8, p.dev, m->comms[0], S.streams[0]);
    }
    const ncclResult_t closed = g_rccl.GroupEnd();
    r.nccl = opened ? opened : (posted ? posted : closed);
    return r;
}

// Before the first real collective: does the hand-declared ABI mean what this file thinks it means?  Rank 0 of the
// communicator sends 16 bytes of a 64-byte pattern to ITSELF (a send / recv pair to one's own rank inside a group is legal
// NCCL) with the datatype constant this file calls ncclUint8 -- if that constant named a wider type, more than 16 bytes
// would move and the guard bytes behind them would change; if the call signatures were off, nothing sensible would arrive.
// With several devices every other rank then exchanges the same 16 bytes with rank 0, so the first gather of a frame is
// not the first time two devices talk.
bool rccl_selftest(rr_multi* m, std::string& why)
{
    const int n = (int)m->devices.size();
    unsigned char pat[64], back[64];
    for (int i = 0; i < 64; i++) pat[i] = (unsigned char)(0xA5 ^ (i * 7));
    std::vector<unsigned char*> src((size_t)n, nullptr), dst((size_t)n, nullptr);
    auto cleanup = [&]() { for (int i = 0; i < n; i++) { (void)hipSetDevice(m->devices[(size_t)i]); if (src[(size_t)i]) (void)hipFree(src[(size_t)i]); if (dst[(size_t)i]) (void)hipFree(dst[(size_t)i]); } (void)hipSetDevice(m->devices[0]); };
    hipError_t e = hipSuccess;
    for (int i = 0; i < n && e == hipSuccess; i++) {
        e = hipSetDevice(m->devices[(size_t)i]);
        if (e == hipSuccess) e = hipMalloc((void**)&src[(size_t)i], 64);
        if (e == hipSuccess) e = hipMalloc((void**)&dst[(size_t)i], 64 * (size_t)(i == 0 ? n : 1));
        if (e == hipSuccess) e = hipMemcpy(src[(size_t)i], pat, 64, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset(dst[(size_t)i], 0, 64 * (size_t)(i == 0 ? n : 1));
    }
    if (e != hipSuccess) { why = std::string("buffers: ") + hipGetErrorString(e); cleanup(); return false; }
    MultiSlot& S = m->slots[0];
    std::vector<Piece> pieces;
    for (int i = 0; i < n; i++) pieces.push_back({ i, src[(size_t)i], dst[0] + 64 * (size_t)i, 16 });       // rank i -> rank 0 (i = 0: to itself), 16 of its 64 bytes
    const GroupError g = send_to_root(m, S, pieces);
    if (g.hip != hipSuccess || g.nccl != 0) {
        why = g.hip != hipSuccess ? std::string("hipSetDevice: ") + hipGetErrorString(g.hip) : std::string("ncclSend / ncclRecv: ") + g_rccl.GetErrorString(g.nccl);
        cleanup(); return false;
    }
    for (int i = 0; i < n && e == hipSuccess; i++) { e = hipSetDevice(m->devices[(size_t)i]); if (e == hipSuccess) e = hipStreamSynchronize(S.streams[(size_t)i]); }
    bool ok = e == hipSuccess;
    if (!ok) why = std::string("synchronize: ") + hipGetErrorString(e);
    (void)hipSetDevice(m->devices[0]);
    for (int i = 0; i < n && ok; i++) {
        if (hipMemcpy(back, dst[0] + 64 * (size_t)i, 64, hipMemcpyDeviceToHost) != hipSuccess) { why = "read-back failed"; ok = false; break; }
        if (std::memcmp(back, pat, 16) != 0) { why = "the 16 bytes rank " + std::to_string(i) + " sent did not arrive"; ok = false; }
        for (int k = 16; k < 64 && ok; k++) if (back[k] != 0) { why = "ncclSend(count = 16, the constant taken for ncclUint8) moved more than 16 bytes: the datatype enum of this librccl differs"; ok = false; }
    }
    cleanup();
    return ok;
}

// batches in flight: 4 streams per device = its 4 hardware queues, the measured optimum of the one-GPU step loop.
// One device: a batch owns no buffers here (its images are assembled in the ctx's frame lane, which delivers them to the
// host itself), so the records outnumber the streams two to one -- a call waits for the batch EIGHT back, long finished,
// rather than for the one its stream ran last
bool create_slots(rr_multi* m)
{
    const size_t n = m->devices.size(), n_streams = (size_t)m->n_streams;
    m->slots.resize((n == 1 && !m->self_rccl) ? 2 * n_streams : n_streams);
    for (size_t si = 0; si < m->slots.size(); si++) {
        MultiSlot& S = m->slots[si];
        S.block.resize(n);
        S.streams.assign(n, nullptr); S.ev_block.assign(n, nullptr);
        bool ok = true;
        S.owns_streams = si < n_streams;
        if (!S.owns_streams) S.streams = m->slots[si - n_streams].streams;
        for (size_t i = 0; i < n && ok; i++)
            ok = hipSetDevice(m->devices[i]) == hipSuccess &&
                 (!S.owns_streams || hipStreamCreateWithFlags(&S.streams[i], hipStreamNonBlocking) == hipSuccess) &&
                 hipEventCreateWithFlags(&S.ev_block[i], hipEventDisableTiming) == hipSuccess;
        ok = ok && hipSetDevice(m->devices[0]) == hipSuccess && hipEventCreateWithFlags(&S.ev_done, hipEventDisableTiming) == hipSuccess &&
             hipHostMalloc((void**)&S.h_bits, sizeof(uint32_t) * n, hipHostMallocDefault) == hipSuccess;
        if (!ok) return false;
        for (size_t i = 0; i < n; i++) S.h_bits[i] = 0;
    }
    return true;
}

// ---- a call: drain / wait, then the stages ---------------------------------------------------------------------
// after an error: nothing of this object may still be in flight when the caller gets the code back (a late D2H copy
// into a buffer the caller frees on error; sticky error bits that would fail the next, healthy call) -- every device is
// drained, its error bits are read and cleared, every slot is free again.  Returns the first error a device reports.
// An error invalidates EVERY batch in flight (advisor, round 4): the drain reads and clears the sticky bits of all frame
// lanes, so a second overflowing batch could no longer be told from a healthy one -- the other pending slots are marked
// failed with `code` and report it from their own rr_multi_wait / the next use of their slot.
int drain_all(rr_multi* m, std::string* first_msg, const MultiSlot* culprit = nullptr, int code = 0)
{
    int first = 0;
    for (size_t i = 0; i < m->ctx.size(); i++) { (void)hipSetDevice(m->devices[i]); (void)hipDeviceSynchronize(); }
    for (size_t i = 0; i < m->ctx.size(); i++) {
        const int rc = rr_synchronize(m->ctx[i], nullptr);
        if (rc && !first) { first = rc; if (first_msg) *first_msg = dev_err(m, i); }
    }
    if (!code) code = first ? first : -7;
    for (MultiSlot& S : m->slots) {
        if (S.pending && &S != culprit) S.failed = code;        // keeps its dst: the wait for that buffer reports it
        else if (!S.failed) S.dst = nullptr;
        S.pending = false;
        for (size_t i = 0; i < m->ctx.size(); i++) S.h_bits[i] = 0;
    }
    return first;
}

// a launch-time failure: keep ITS message, but hand the object back drained
int fail_drained(rr_multi* m, int code, const std::string& msg)
{
    (void)drain_all(m, nullptr, nullptr, code);
    return mfail(m, code, msg);
}
#define RRM_TRY_HIP(m, expr) \
    do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail_drained((m), -100, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

int wait_slot(rr_multi* m, MultiSlot& S)
{
    if (S.failed) {
        const int rc = S.failed;
        S.failed = 0; S.dst = nullptr;
        return mfail(m, rc, "this batch was in flight when another batch's error drained the object: its images are invalid (an error invalidates every batch in flight)");
    }
    if (!S.pending) return 0;
    const int n = (int)m->ctx.size();
    hipError_t e = hipSetDevice(m->devices[0]);
    if (e == hipSuccess) {
        // one device: the image may still sit on its frame lane or be on its way over SDMA (rr_simulate_batch_host_async);
        // several: the root's copy is an rr_deliver_to_host_async job -- either way the context's fence completes it
        if (rr_wait_host(m->ctx[0], S.dst)) return fail_drained(m, -100, dev_err(m, 0));
    }
    if (e == hipSuccess) e = hipEventSynchronize(S.ev_done);
    if (e != hipSuccess) return fail_drained(m, -100, std::string("rr_multi_wait: ") + hipGetErrorString(e));
    S.pending = false; S.dst = nullptr;
    // the root's stream is ordered behind every device's block (collective / events), each block behind its error bits
    uint32_t bits = 0;
    for (int i = 0; i < n; i++) bits |= S.h_bits[i];
    if (bits) {
        std::string msg;
        const int code = (bits & 1u) ? -7 : -8;
        const int rc = drain_all(m, &msg, &S, code);
        return mfail(m, rc ? rc : code, rc ? msg : "a device reported an overflow / bad id");
    }
    return 0;
}

// one call on its slot, laid out by ONE rr_multi_plan call: what renders, what travels and what the root assembles all
// follow from these
struct Call {
    MultiSlot& S;
    const float* poses; int n_frames; uint8_t* out;
    int equal; size_t per;                // equal_blocks, bytes_per_device
    const size_t *so, *ro, *pb;           // send_off, recv_off, piece_bytes: [n_devices][n_frames]
};
struct BlockResult { int rc = 0; std::string hip; };      // rc of the context, or -100 with the HIP error's text

// one device: no collective; the images take the ctx's own host delivery (SDMA at once behind the batch, or the
// stream-ordered copy: rr_simulate_batch_host_async)
int single_device(rr_multi* m, MultiSlot& S, const float* poses, int n_frames, uint8_t* out)
{
    RRM_TRY_HIP(m, hipSetDevice(m->devices[0]));
    int rc = rr_simulate_batch_host_async(m->ctx[0], poses, n_frames, out, S.streams[0]);
    if (rc) return fail_drained(m, rc, dev_err(m, 0));
    rc = rr_peek_error_bits_async(m->ctx[0], &S.h_bits[0], S.streams[0]);
    if (rc) return fail_drained(m, rc, dev_err(m, 0));
    const hipError_t e = hipEventRecord(S.ev_done, S.streams[0]);
    if (e != hipSuccess) return fail_drained(m, -100, std::string("hipEventRecord: ") + hipGetErrorString(e));
    return 0;
}

// device entry d renders its block of all frames in one set of launches on its stream of the slot.  Its columns are
// where the plan puts its piece of frame 0: they begin at recv_off / n_cells and are piece_bytes / n_cells many
BlockResult render_block(rr_multi* m, const Call& K, size_t d)
{
    MultiSlot& S = K.S;
    const size_t k0 = d * (size_t)K.n_frames, C = (size_t)m->cfg.n_cells;
    const int b = (int)(K.ro[k0] / C), e = b + (int)(K.pb[k0] / C);
    BlockResult r;
    hipError_t he = hipSetDevice(m->devices[d]);
    if (he == hipSuccess) he = S.block[d].ensure(std::max<size_t>(1, (size_t)K.n_frames * K.pb[k0]));
    S.h_bits[d] = 0;
    if (he == hipSuccess && e > b) {
        rr_ctx* c = m->ctx[d];
        { rr::HostProfScope hp(10, "multi: device entry: render"); r.rc = rr_simulate_batch_columns_device(c, K.poses, K.n_frames, b, e, S.block[d].p, S.streams[d]); }
        { rr::HostProfScope hp(11, "multi: device entry: error bits"); if (!r.rc) r.rc = rr_peek_error_bits_async(c, &S.h_bits[d], S.streams[d]); }
        if (r.rc) return r;
    }
    { rr::HostProfScope hp(12, "multi: device entry: block event"); if (he == hipSuccess) he = hipEventRecord(S.ev_block[d], S.streams[d]); }
    if (he != hipSuccess) { r.rc = -100; r.hip = hipGetErrorString(he); }
    return r;
}

// 1. every device renders its block (all devices concurrently): each entry's launches from its own enqueue thread where
//    there are workers, otherwise from the caller's thread, which stops at the first entry that fails
std::vector<BlockResult> render_blocks(rr_multi* m, const Call& K)
{
    const size_t n = m->ctx.size();
    std::vector<BlockResult> res(n);
    const auto one = [&](size_t i) { res[i] = render_block(m, K, i); };
    for (size_t i = 0; m->workers.empty() && i < n && (i == 0 || res[i - 1].rc == 0); i++) one(i);
    for (size_t i = 0; i < m->workers.size(); i++) post(m->workers[i].get(), [&one, i] { one(i); });
    for (size_t i = 0; i < m->workers.size(); i++) collect(m->workers[i].get());
    return res;
}

// 2. ONE collective: a GATHER to the root (device 0), nobody else receives anything.  RCCL has no plain gather in
//    every version, so it is one group of send / recv pairs along the plan: equal blocks travel as one piece per device
//    into [device][frame][n_loc][n_cells], ragged ones frame by frame into [frame][n_angles][n_cells].  The root's own
//    pieces (and, in loopback, everybody's) are plain copies on the root's stream, ahead of the group
int gather_blocks(rr_multi* m, const Call& K)
{
    MultiSlot& S = K.S;
    const size_t n = m->ctx.size(), F = (size_t)K.n_frames;
    RRM_TRY_HIP(m, hipSetDevice(m->devices[0]));
    RRM_TRY_HIP(m, S.gathered.ensure(K.equal ? n * K.per : F * (size_t)m->cfg.n_angles * (size_t)m->cfg.n_cells));
    std::vector<Piece> wire;               // what goes through RCCL
    for (size_t i = 0; i < n; i++) for (size_t f = 0; f < (K.equal ? 1 : F); f++) {
        const size_t k = i * F + f;
        const Piece p = K.equal ? Piece{ (int)i, S.block[i].p, S.gathered.p + i * K.per, K.per }
                                : Piece{ (int)i, S.block[i].p + K.so[k], S.gathered.p + K.ro[k], K.pb[k] };
        if (!p.bytes) continue;
        if ((i == 0 && !m->self_rccl) || m->loopback) {
            if (i != 0) RRM_TRY_HIP(m, hipStreamWaitEvent(S.streams[0], S.ev_block[i], 0));
            RRM_TRY_HIP(m, hipMemcpyAsync(p.dst, p.src, p.bytes, hipMemcpyDeviceToDevice, S.streams[0]));
        } else wire.push_back(p);
    }
    if (m->loopback) return 0;
    const GroupError g = send_to_root(m, S, wire);
    if (g.hip != hipSuccess) return fail_drained(m, -100, std::string("hipSetDevice (collective): ") + hipGetErrorString(g.hip));
    if (g.nccl != 0) return fail_drained(m, -101, std::string("ncclSend / ncclRecv: ") + g_rccl.GetErrorString(g.nccl));
    return 0;
}

// 3. root: transpose what was gathered into mono8 images, copy them to the caller's host buffer
int deliver_root(rr_multi* m, const Call& K)
{
    MultiSlot& S = K.S;
    const size_t A = (size_t)m->cfg.n_angles, C = (size_t)m->cfg.n_cells, bytes = (size_t)K.n_frames * C * A;
    const size_t frame_stride = K.equal ? K.per / (size_t)K.n_frames : A * C, block_stride = K.equal ? K.per : A * C;
    RRM_TRY_HIP(m, hipSetDevice(m->devices[0]));
    RRM_TRY_HIP(m, S.d_imgs.ensure(bytes));
    int rc = rr_assemble_frames_device(m->ctx[0], S.gathered.p, (int)(frame_stride / C), block_stride, K.n_frames, frame_stride, S.d_imgs.p, S.streams[0]);
    // (over the SDMA engines, whichever HIP runtime serves the process: rr_deliver_to_host_async; fenced in wait_slot)
    if (!rc) rc = rr_deliver_to_host_async(m->ctx[0], S.d_imgs.p, K.out, bytes, S.streams[0]);
    if (rc) return fail_drained(m, rc, std::string("root: ") + rr_last_error(m->ctx[0]));
    RRM_TRY_HIP(m, hipEventRecord(S.ev_done, S.streams[0]));
    return 0;
}

}  // namespace

extern "C" {

rr_multi* rr_create_multi(const int* devices, int n_devices)
{
    if (!devices || n_devices < 1 || n_devices > 64) { g_multi_create_error = "rr_create_multi: need 1..64 device indices"; return nullptr; }
    rr_multi* m = new rr_multi();
    const auto fail = [m](const std::string& msg) -> rr_multi* { g_multi_create_error = msg; rr_destroy_multi(m); return nullptr; };
    // RR_MULTI_LOOPBACK=1 (tests on a one-GPU box): a device may be listed several times; every listed entry gets its own
    // context, block and stream as usual, and the ONE collective of a call is replaced by device-to-device copies that
    // follow the same plan (rr_multi_plan) -- everything of the n > 1 path runs except the RCCL calls themselves
    m->loopback = env_int(getenv("RR_MULTI_LOOPBACK"), 0) != 0;
    m->n_streams = std::max(1, std::min(env_int(getenv("RR_MULTI_SLOTS"), 4), 8));
    // RR_MULTI_SELF_RCCL=1 (test switch for one-GPU boxes, the complement of the loopback): ONE device whose block goes
    // through the REAL RCCL calls -- ncclCommInitAll with one rank, one group of ncclSend / ncclRecv to itself on the slot's
    // stream -- instead of the single-device route: what the loopback leaves out (library loading, symbols, datatype,
    // group semantics, stream ordering of the collective against render and transpose) runs here
    const int self_rccl = (n_devices == 1 && !m->loopback) ? env_int(getenv("RR_MULTI_SELF_RCCL"), 0) : 0;
    m->self_rccl = self_rccl != 0; m->self_rccl_frames = self_rccl == 2;
    m->threads = n_devices > 1 && env_int(getenv("RR_MULTI_THREADS"), 0) != 0;
    for (int i = 0; i < n_devices && !m->loopback; i++) for (int j = 0; j < i; j++)
        if (devices[i] == devices[j]) return fail("rr_create_multi: a device is listed twice");
    m->devices.assign(devices, devices + n_devices);
    rr_default_config(&m->cfg);
    for (int i = 0; i < n_devices; i++) {
        rr_ctx* c = rr_create(devices[i]);
        if (!c) return fail(std::string("rr_create_multi: ") + rr_last_error(nullptr));
        m->ctx.push_back(c);
    }
    if (!create_slots(m)) return fail("rr_create_multi: stream / event creation failed");
    if (m->threads) start_workers(m);
    if ((n_devices > 1 && !m->loopback) || m->self_rccl) {
        // the communicator is owned here: one rank per device of this process
        std::string why;
        if (!g_rccl.load(why)) return fail(why);
        m->comms.resize((size_t)n_devices, nullptr);
        const ncclResult_t r = g_rccl.CommInitAll(m->comms.data(), n_devices, devices);
        if (r != 0) { m->comms.clear(); return fail(std::string("rr_create_multi: ncclCommInitAll: ") + g_rccl.GetErrorString(r)); }
        if (!rccl_selftest(m, why)) return fail("rr_create_multi: RCCL self-test failed: " + why);
    }
    return m;
}

void rr_destroy_multi(rr_multi* m)
{
    if (!m) return;
    m->workers.clear();           // (joins the enqueue threads)
    // the root's deliveries (rr_deliver_to_host_async: SDMA copies issued by a worker thread, which no device sync waits for)
    // may still read slot buffers: fence them before any slot buffer or stream goes
    if (!m->ctx.empty()) (void)rr_wait_host(m->ctx[0], nullptr);
    for (size_t i = 0; i < m->ctx.size(); i++) { (void)hipSetDevice(m->devices[i]); (void)hipDeviceSynchronize(); }
    for (size_t i = 0; i < m->comms.size(); i++) if (m->comms[i]) g_rccl.CommDestroy(m->comms[i]);
    for (MultiSlot& S : m->slots) {
        for (size_t i = 0; i < S.streams.size(); i++) {
            (void)hipSetDevice(m->devices[i]);
            if (S.ev_block[i]) (void)hipEventDestroy(S.ev_block[i]);
            if (S.owns_streams && S.streams[i]) (void)hipStreamDestroy(S.streams[i]);
        }
        (void)hipSetDevice(m->devices[0]);
        if (S.ev_done) (void)hipEventDestroy(S.ev_done);
        if (S.h_bits) (void)hipHostFree(S.h_bits);
    }
    m->slots.clear();             // the slots' buffers go here, ahead of their devices' contexts (hipFree finds a pointer's device itself)
    for (size_t i = 0; i < m->ctx.size(); i++) rr_destroy(m->ctx[i]);
    delete m;
}

const char* rr_multi_last_error(const rr_multi* m) { return m ? m->err.c_str() : g_multi_create_error.c_str(); }
int rr_multi_device_count(const rr_multi* m) { return m ? (int)m->ctx.size() : 0; }
int rr_multi_rccl_version(const rr_multi* m) { return (m && !m->comms.empty()) ? g_rccl.version : 0; }
rr_ctx* rr_multi_ctx(rr_multi* m, int i) { return (m && i >= 0 && (size_t)i < m->ctx.size()) ? m->ctx[(size_t)i] : nullptr; }

// ---- replicated state: every setter goes to every device ------------------------------------------------
int rr_multi_set_mesh(rr_multi* m, const float* verts, size_t nv, const uint32_t* faces, size_t nf, const uint32_t* face_object_id)
{
    return replicate_tree(m, [&](rr_ctx* c) { return rr_set_mesh(c, verts, nv, faces, nf, face_object_id); });
}
int rr_multi_set_mesh_gpu(rr_multi* m, const float* verts, size_t nv, const uint32_t* faces, size_t nf, const uint32_t* face_object_id)
{
    return replicate_tree(m, [&](rr_ctx* c) { return rr_set_mesh_gpu(c, verts, nv, faces, nf, face_object_id); });
}
// dynamic scenes: every device holds the same rest geometry and poses (rr_copy_mesh copies them), so a pose or vertex
// update is the same refit on each; a rebuild runs once and the finished tree travels as rr_multi_set_mesh's does
int rr_multi_set_object_poses(rr_multi* m, const float* poses, size_t n)
{
    return on_each(m, [&](rr_ctx* c, size_t) { return rr_set_object_poses(c, poses, n); });
}
int rr_multi_update_vertices(rr_multi* m, const float* verts, size_t nv)
{
    return on_each(m, [&](rr_ctx* c, size_t) { return rr_update_vertices(c, verts, nv); });
}
int rr_multi_rebuild_tree(rr_multi* m, int builder)
{
    return replicate_tree(m, [&](rr_ctx* c) { return rr_rebuild_tree(c, builder); });
}
int rr_multi_set_materials(rr_multi* m, const rr_material* materials, size_t n_materials,
                           const int32_t* object_materials, size_t n_objects, int32_t material_id_air)
{
    return on_each(m, [&](rr_ctx* c, size_t) { return rr_set_materials(c, materials, n_materials, object_materials, n_objects, material_id_air); });
}
int rr_multi_set_config(rr_multi* m, const rr_config* cfg)
{
    if (!m) return -1;
    if (!cfg) return mfail(m, -3, "rr_multi_set_config: null config");
    const int rc = on_each(m, [&](rr_ctx* c, size_t) { return rr_set_config(c, cfg); });
    if (!rc) { m->cfg = *cfg; m->have_cfg = true; }
    return rc;
}
int rr_multi_set_beam_samples(rr_multi* m, const float* dirs, size_t n)
{
    return on_each(m, [&](rr_ctx* c, size_t) { return rr_set_beam_samples(c, dirs, n); });
}
int rr_multi_set_noise_offsets(rr_multi* m, const float* rnd, size_t n)
{
    return on_each(m, [&](rr_ctx* c, size_t) { return rr_set_noise_offsets(c, rnd, n); });
}
int rr_multi_set_motion_poses(rr_multi* m, const float* poses, size_t n)
{
    return on_each(m, [&](rr_ctx* c, size_t) { return rr_set_motion_poses(c, poses, n); });
}

// ---- the data plan of one call: pure arithmetic, exported so that it can be checked without a GPU ------------
// equal blocks : device r's whole block buffer (`bytes_per_device`) travels as ONE piece and lands at r * bytes_per_device
//                of the root's buffer, laid out [device][frame][n_loc][n_cells]
// ragged blocks: device r sends, for every frame f, the n_loc_r * n_cells bytes at send_off[r][f] of ITS block buffer
//                ([frame][n_loc_r][n_cells]) to the root, which receives them at recv_off[r][f] of [frame][n_angles][n_cells]
int rr_multi_plan(int n_angles, int n_cells, int n_devices, int n_frames, int* equal_blocks, size_t* bytes_per_device,
                  size_t* send_off, size_t* recv_off, size_t* piece_bytes)
{
    if (n_angles < 1 || n_cells < 1 || n_devices < 1 || n_frames < 1) return -3;
    bool equal = true; int b0 = 0, e0 = 0;
    rr_partition(n_angles, n_devices, 0, &b0, &e0);
    for (int r = 0; r < n_devices; r++) {
        int b = 0, e = 0; rr_partition(n_angles, n_devices, r, &b, &e);
        equal = equal && (e - b) == (e0 - b0);
        for (int f = 0; f < n_frames; f++) {
            const size_t k = (size_t)r * n_frames + f;
            if (send_off) send_off[k] = (size_t)f * (size_t)(e - b) * n_cells;
            if (recv_off) recv_off[k] = ((size_t)f * n_angles + (size_t)b) * n_cells;
            if (piece_bytes) piece_bytes[k] = (size_t)(e - b) * n_cells;
        }
    }
    if (equal_blocks) *equal_blocks = equal ? 1 : 0;
    if (bytes_per_device) *bytes_per_device = (size_t)n_frames * (size_t)(e0 - b0) * n_cells;
    return 0;
}

// ---- frames ------------------------------------------------------------------------------------------------
int rr_multi_wait(rr_multi* m, const void* h_imgs_u8)
{
    if (!m) return -1;
    // oldest first, so that an error is reported for the batch that caused it
    int first = 0;
    for (size_t k = 0; k < m->slots.size(); k++) {
        MultiSlot& S = m->slots[(m->next_slot + k) % m->slots.size()];
        if ((!S.pending && !S.failed) || (h_imgs_u8 && S.dst != h_imgs_u8)) continue;
        const int rc = wait_slot(m, S);
        if (rc) { if (!first) first = rc; break; }       // (a failed wait drained everything)
    }
    // "every outstanding batch": the error is reported once for all of them
    if (!h_imgs_u8 && first) for (MultiSlot& S : m->slots) if (S.failed) { S.failed = 0; S.dst = nullptr; }
    return first;
}

int rr_multi_simulate_batch_async(rr_multi* m, const float* poses, int n_frames, uint8_t* out_imgs_u8)
{
    if (!m) return -1;
    if (!m->have_cfg) return mfail(m, -2, "rr_multi_set_config has not been called");
    if (!poses || !out_imgs_u8) return mfail(m, -3, "rr_multi_simulate_batch: null poses/output");
    if (n_frames < 1 || n_frames > RR_MAX_BATCH) return mfail(m, -3, "rr_multi_simulate_batch: n_frames must be 1..64");
    const size_t n = m->ctx.size();
    MultiSlot& S = m->slots[m->next_slot];
    m->next_slot = (m->next_slot + 1) % m->slots.size();
    rr::HostProfScope hp_all(8, "multi: whole call");
    { rr::HostProfScope hp(9, "multi: wait for the slot"); const int rc = wait_slot(m, S); if (rc) return rc; }        // the batch that used this slot's buffers last
    if (n == 1 && !m->self_rccl) {
        const int rc = single_device(m, S, poses, n_frames, out_imgs_u8);
        if (rc) return rc;
    } else {
        const size_t nF = n * (size_t)n_frames;
        std::vector<size_t> off(3 * nF);
        Call K{ S, poses, n_frames, out_imgs_u8, 0, 0, off.data(), off.data() + nF, off.data() + 2 * nF };
        (void)rr_multi_plan(m->cfg.n_angles, m->cfg.n_cells, (int)n, n_frames, &K.equal, &K.per, off.data(), off.data() + nF, off.data() + 2 * nF);
        if (m->self_rccl_frames) K.equal = 0;      // (test switch: one send / recv pair per frame, as ragged blocks travel)
        const std::vector<BlockResult> res = render_blocks(m, K);
        for (size_t i = 0; i < n; i++) if (res[i].rc) return fail_drained(m, res[i].rc, dev_err(m, i, res[i].hip));
        rr::HostProfScope hp_root(13, "multi: gather + assemble + D2H");
        int rc = gather_blocks(m, K);
        if (!rc) rc = deliver_root(m, K);
        if (rc) return rc;
    }
    S.pending = true; S.dst = out_imgs_u8;
    return 0;
}

int rr_multi_simulate_batch(rr_multi* m, const float* poses, int n_frames, uint8_t* out_imgs_u8)
{
    const int rc = rr_multi_simulate_batch_async(m, poses, n_frames, out_imgs_u8);
    if (rc) return rc;
    return rr_multi_wait(m, out_imgs_u8);
}

int rr_multi_simulate(rr_multi* m, const float pose_qxyzw_t[7], uint8_t* out_u8)
{
    return rr_multi_simulate_batch(m, pose_qxyzw_t, 1, out_u8);
}

}  // extern "C"
