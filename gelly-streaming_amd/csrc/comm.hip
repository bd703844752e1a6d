// comm.hip — the multi-GPU CombineCC under the C ABI: gs_comm_* and gs_cc_merge_window.
//
// Replaces the reference's two exchanges of partial summaries (paths relative to the reference's
// src/main/java/org/apache/flink/graph/streaming/):
//   * the windowAll gather of every partition's window result to the parallelism-1 reduce and
//     Merger (SummaryBulkAggregation.java:81-83, SummaryAggregation.java:106-119), and
//   * ConnectedComponentsTree's pairwise tree, partials keyed by partition / 2 per round
//     (SummaryTreeReduce.java:95-123).
// One process per GPU; one RCCL communicator per rank (ncclCommInitRank from a unique id that
// rank 0 makes and the caller distributes, the way torch.distributed or a Flink job's
// configuration would). A partial summary crosses the wire as a DELTA: the (vertex, root) pairs
// of every root this rank hooked since its last export (gs_cc_export_marks), 8 B per pair;
// folding a delta (= DisjointSet.merge over its pairs, DisjointSet.java:127-131) carries every
// component join of that rank's window into another summary.
//
// Transports: RCCL over xGMI (production), or an in-process group of handles on one device driven
// by one thread per rank (gs_comm_create_local: the same exchange code, collectives done with
// device-to-device copies ordered by HIP events and host barriers) for tests on a one-GPU box,
// where RCCL refuses two ranks on one device.
//
// What two ranks must compute alike (slot sizes, exact or speculative rounds, the broadcast
// schedule, the tree's pairing) is host arithmetic in exchange_plan.hpp, checked on a CPU.
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "cc_internal.hpp"
#include "exchange_plan.hpp"
#include "owned.hpp"

namespace gsgpu {

namespace {

// pairs [n, m) of buf = copies of pair 0 (a repeated union is a no-op): fixed-size slots for the
// all-gather. P = uint2 (dense (vertex, root) uint32 pairs) or P16 (sparse (id, root id) int64
// pairs, 8-B aligned inside count-headed slots)
struct P16 { unsigned long long a, b; };
template <typename P>
__global__ void k_pad_pairs(P* __restrict__ buf, uint64_t n, uint64_t m) {
    const P p = buf[0];
    for (uint64_t i = n + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (uint64_t)gridDim.x * blockDim.x)
        buf[i] = p;
}
void pad_pairs(bool sparse, uint32_t* buf, uint64_t n, uint64_t m, hipStream_t s) {
    const dim3 grid((unsigned)std::min<uint64_t>((m - n + 255) / 256, 4096));
    if (sparse) hipLaunchKernelGGL(k_pad_pairs<P16>, grid, dim3(256), 0, s, reinterpret_cast<P16*>(buf), n, m);
    else hipLaunchKernelGGL(k_pad_pairs<uint2>, grid, dim3(256), 0, s, reinterpret_cast<uint2*>(buf), n, m);
}
// bytes / 32-bit words per exported pair
inline uint64_t pbytes(const CcInfo& in) { return in.sparse ? 16 : 8; }
inline uint64_t pwords(const CcInfo& in) { return in.sparse ? 4 : 2; }

// ---- in-process group (tests): threads on one device ----
struct LocalGroup {
    explicit LocalGroup(int w) : world(w), send(w, nullptr), ev(w, nullptr), done(w, nullptr), box((size_t)w * w) {}
    int world;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t gen = 0;
    std::vector<const void*> send;
    std::vector<hipEvent_t> ev, done;             // per rank: data ready / peers' reads done
    struct Box {                                   // point-to-point mailbox src -> dst
        const void* p = nullptr;
        size_t bytes = 0;
        hipEvent_t ready = nullptr, taken = nullptr;
        int state = 0;                             // 0 empty, 1 posted, 2 copied
    };
    std::vector<Box> box;
    bool failed = false;                           // a rank's exchange failed: every wait returns
    // false when the group has failed (the caller returns GS_ERR_COMM instead of hanging)
    bool barrier() {
        std::unique_lock<std::mutex> lk(mu);
        if (failed) return false;
        const uint64_t g = gen;
        if (++arrived == world) {
            arrived = 0;
            ++gen;
            cv.notify_all();
        } else {
            cv.wait(lk, [&] { return gen != g || failed; });
        }
        return !failed;
    }
    void fail_all() {
        std::lock_guard<std::mutex> lk(mu);
        failed = true;
        cv.notify_all();
    }
};

}  // namespace
}  // namespace gsgpu

using namespace gsgpu;

struct gs_comm {
    // ---- transport and buffers: live as long as the communicator ----
    int rank = 0, world = 1, device = 0;
    ncclComm_t nccl = nullptr;                     // RCCL transport
    std::shared_ptr<LocalGroup> local;             // or the in-process group
    // prefilter, asynchronous filter-state broadcasts: their own communicator (RCCL: split from the
    // main one at bind; in-process: the same group)
    ncclComm_t nccl_side = nullptr;
    Stream side;                                   // copies the slots' count words to the host
    Event ev_ready, ev_done;
    Event ev_slots;                                // a speculative round's slots have arrived
    Event ev_counts;                               // their count words are on the host
    // exchange buffers (device), sized at the first merge for the handle's capacity
    uint64_t cap_pairs = 0;
    uint64_t pair_bytes = 0;                       // 8: dense (uint32 vertex, root); 16: sparse (int64 ids)
    DevBuf<uint32_t> sendbuf;                      // cap_pairs pairs (2 x the handle's capacity)
    uint64_t send_pairs = 0;                       // pairs each send buffer holds (count word included):
                                                   // cap_pairs + 1, more for a prefilter sender's big slice
    DevBuf<uint32_t> sendbuf2;                     // exports alternate between the two, so a pending
                                                   // window's tail survives the next export
    DevBuf<uint32_t> recvbuf;                      // exact rounds and tails: grows to what arrives
    DevBuf<uint32_t> slotbuf;                      // speculative rounds: world count-headed slots
    DevBuf<unsigned long long> dcnt;               // [world + 1]: gathered counts, [world] own/received
    Pinned<unsigned long long> hcnt;               // pinned mirror
    DevBuf<uint32_t> bword;                        // the synchronous broadcast's giant slot words (device, 2)
    struct Bcast {                                 // the asynchronous broadcasts' stream, events and staging,
        Stream bside;                              // made on the first one
        DevBuf<uint32_t> bstage;                   // rank 0: a snapshot [gbits | 2 giant words]; senders: 2 slots
        Event ev_bmain;                            // senders: a slot is free (its install ran); rank 0: the
                                                   // last broadcast has read the snapshot
        Event ev_brecv[2];                         // senders: slot k has arrived; rank 0 ([0]): snapshot taken
        int create(size_t words) {
            GS_TRY(bside.create());
            GS_TRY(ev_bmain.create());
            GS_TRY(ev_brecv[0].create());
            GS_TRY(ev_brecv[1].create());
            return bstage.grow(words, "filter-state broadcast staging");
        }
    } bc;
    uint64_t bslot_words = 0;                      // 32-bit words per staging slot
    gs_cc_t* bound = nullptr;                      // the one handle and mode this communicator serves
    int mode = -1;
    uint64_t reset_gen = 0;                        // the handle's reset generation of the current stream
    bool broken = false;                           // an exchange failed: the communicator is unusable
    // Per-stream in spirit, but kept across a reset: gs_cc_reset leaves the handle's marking as it is
    // (rank 0's stays off), and the last delta is only the next export's size hint.
    bool root_marking_off = false;
    uint64_t last_delta = 0;                       // the largest delta of the last verified window
    uint64_t bytes_sent = 0, bytes_recv = 0, exchanges = 0, overflows = 0;
    // ---- the current stream: a reset of the handle starts a new one from StreamState() ----
    struct StreamState {
        uint64_t spec_slot = 0;                    // allgather: slot size of the next speculative round (0: exact)
        std::vector<uint64_t> gslot;               // gather to rank 0: every sender's slot (empty: none sized yet)
        uint64_t win = 0;                          // prefilter: windows so far (exact young rounds, broadcast schedule)
        int64_t bpend[2] = {-1, -1};               // prefilter senders: the window whose state staging slot k holds
    } st;                                          // (-1: none; a broadcast in flight at a reset lands unused)
    // ---- the one window whose speculative round is not verified yet: it outlives a reset (its
    // verification is a collective the peers are in) and is settled first ----
    struct Pending {
        bool open = false;
        uint64_t slot = 0;                         // the slot size S it was sent with
        uint32_t* buf = nullptr;                   // the last export's send buffer: the tail [S, n) is sent from
    } pend;                                        // it, and the next export goes into the other one
};

namespace {

int nccl_fail(ncclResult_t r, const char* what) {
    return fail(GS_ERR_COMM, "%s failed: %s", what, ncclGetErrorString(r));
}
#define GS_NCCL(expr)                                                                        \
    do {                                                                                     \
        ncclResult_t r_ = (expr);                                                            \
        if (r_ != ncclSuccess) return nccl_fail(r_, #expr);                                  \
    } while (0)

// ---- the collective primitives the exchanges need ----
int allgather(gs_comm_t* c, const void* send, void* recv, size_t bytes, hipStream_t s) {
    if (c->nccl) {
        GS_NCCL(ncclAllGather(send, recv, bytes, ncclUint8, c->nccl, s));
        return GS_OK;
    }
    LocalGroup& g = *c->local;
    GS_HIP(hipEventRecord(c->ev_ready, s));
    g.send[c->rank] = send;
    g.ev[c->rank] = c->ev_ready;
    if (!g.barrier()) return fail(GS_ERR_COMM, "in-process group: a peer's exchange failed");   // buffers published
    for (int q = 0; q < c->world; ++q) {
        if (q != c->rank) GS_HIP(hipStreamWaitEvent(s, g.ev[q], 0));
        GS_HIP(hipMemcpyAsync(static_cast<char*>(recv) + (size_t)q * bytes, g.send[q], bytes, hipMemcpyDeviceToDevice, s));
    }
    GS_HIP(hipEventRecord(c->ev_done, s));
    g.done[c->rank] = c->ev_done;
    if (!g.barrier()) return fail(GS_ERR_COMM, "in-process group: a peer's exchange failed");   // reads enqueued
    for (int q = 0; q < c->world; ++q)             // a send buffer is rewritten only after the
        if (q != c->rank) GS_HIP(hipStreamWaitEvent(s, g.done[q], 0));   // peers' reads of it
    return GS_OK;
}

int send(gs_comm_t* c, const void* p, size_t bytes, int peer, hipStream_t s) {
    if (c->nccl) {
        GS_NCCL(ncclSend(p, bytes, ncclUint8, peer, c->nccl, s));
        return GS_OK;
    }
    LocalGroup& g = *c->local;
    LocalGroup::Box& b = g.box[(size_t)c->rank * c->world + peer];
    GS_HIP(hipEventRecord(c->ev_ready, s));
    std::unique_lock<std::mutex> lk(g.mu);
    b.p = p;
    b.bytes = bytes;
    b.ready = c->ev_ready;
    b.state = 1;
    g.cv.notify_all();
    g.cv.wait(lk, [&] { return b.state == 2 || g.failed; });   // the receiver has enqueued its copy
    if (b.state != 2) return fail(GS_ERR_COMM, "in-process group: a peer's exchange failed");
    b.state = 0;
    const hipEvent_t taken = b.taken;
    lk.unlock();
    if (!taken) return fail(GS_ERR_COMM, "local send of %zu bytes to rank %d: the receiver refused it", bytes, peer);
    GS_HIP(hipStreamWaitEvent(s, taken, 0));       // p is reused only after the copy ran
    return GS_OK;
}

int recv(gs_comm_t* c, void* p, size_t bytes, int peer, hipStream_t s) {
    if (c->nccl) {
        GS_NCCL(ncclRecv(p, bytes, ncclUint8, peer, c->nccl, s));
        return GS_OK;
    }
    LocalGroup& g = *c->local;
    LocalGroup::Box& b = g.box[(size_t)peer * c->world + c->rank];
    std::unique_lock<std::mutex> lk(g.mu);
    g.cv.wait(lk, [&] { return b.state == 1 || g.failed; });
    if (b.state != 1) return fail(GS_ERR_COMM, "in-process group: a peer's exchange failed");
    if (b.bytes != bytes) {
        b.taken = nullptr;
        b.state = 2;
        g.cv.notify_all();
        return fail(GS_ERR_COMM, "local recv of %zu bytes from rank %d, %zu sent", bytes, peer, b.bytes);
    }
    GS_HIP(hipStreamWaitEvent(s, b.ready, 0));
    GS_HIP(hipMemcpyAsync(p, b.p, bytes, hipMemcpyDeviceToDevice, s));
    GS_HIP(hipEventRecord(c->ev_done, s));
    b.taken = c->ev_done;
    b.state = 2;
    g.cv.notify_all();
    return GS_OK;
}

// rank 0's buffer into every rank's buffer of the same address role, in place (side: on the
// prefilter's broadcast communicator; the in-process group serves both, its host barriers order them)
int bcast(gs_comm_t* c, void* buf, size_t bytes, hipStream_t s, bool side = false) {
    if (c->nccl) {
        GS_NCCL(ncclBroadcast(buf, buf, bytes, ncclUint8, 0, side ? c->nccl_side : c->nccl, s));
        return GS_OK;
    }
    LocalGroup& g = *c->local;
    GS_HIP(hipEventRecord(c->ev_ready, s));
    g.send[c->rank] = buf;
    g.ev[c->rank] = c->ev_ready;
    if (!g.barrier()) return fail(GS_ERR_COMM, "in-process group: a peer's exchange failed");
    if (c->rank != 0) {
        GS_HIP(hipStreamWaitEvent(s, g.ev[0], 0));
        GS_HIP(hipMemcpyAsync(buf, g.send[0], bytes, hipMemcpyDeviceToDevice, s));
    }
    GS_HIP(hipEventRecord(c->ev_done, s));
    g.done[c->rank] = c->ev_done;
    if (!g.barrier()) return fail(GS_ERR_COMM, "in-process group: a peer's exchange failed");
    if (c->rank == 0)                              // rank 0's buffer changes only after the copies
        for (int q = 1; q < c->world; ++q) GS_HIP(hipStreamWaitEvent(s, g.done[q], 0));
    return GS_OK;
}

struct Group {                                     // ncclGroupStart/End around p2p batches
    gs_comm_t* c;
    explicit Group(gs_comm_t* c_) : c(c_) { if (c->nccl) (void)ncclGroupStart(); }
    int end() {
        if (c->nccl) GS_NCCL(ncclGroupEnd());
        c = nullptr;
        return GS_OK;
    }
    ~Group() { if (c && c->nccl) (void)ncclGroupEnd(); }
};

// Grows a receive or slot buffer to `bytes`. Folds already enqueued on the stream may still read
// the old one (a receive buffer is read by the fold kernels that follow its collective), so the
// stream drains before the free.
int ensure(DevBuf<uint32_t>& b, size_t bytes, hipStream_t s) { return b.grow((bytes + 3) / 4, "exchange buffer", s); }

// ---- the pieces every exchange is made of ----

// Every rank's word `mine` into hcnt[0, world) on every rank (the host waits for it).
int allgather_word(gs_comm_t* c, unsigned long long mine, hipStream_t s) {
    const int P = c->world;
    c->hcnt[P] = mine;                               // (pinned: the copy reads it when it runs)
    GS_HIP(hipMemcpyAsync(c->dcnt + P, c->hcnt + P, sizeof(unsigned long long), hipMemcpyHostToDevice, s));
    GS_TRY(allgather(c, c->dcnt + P, c->dcnt, sizeof(unsigned long long), s));
    GS_HIP(hipMemcpyAsync(c->hcnt, c->dcnt, P * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    GS_HIP(hipStreamSynchronize(s));
    return GS_OK;
}

// A speculative round's count words (n of them, `stride` bytes apart from `src`) go to the host at
// `dst` on the side stream, so the fold and the close start right after the collective; the
// window's verification waits for ev_counts and reads them (the next window's collective is
// enqueued only after that, so the slots are not overwritten under the copy).
int counts_aside(gs_comm_t* c, const void* src, size_t stride, int n, unsigned long long* dst, hipStream_t s) {
    const size_t w = sizeof(unsigned long long);
    GS_HIP(hipEventRecord(c->ev_slots, s));
    GS_HIP(hipStreamWaitEvent(c->side, c->ev_slots, 0));
    if (n == 1) GS_HIP(hipMemcpyAsync(dst, src, w, hipMemcpyDeviceToHost, c->side));
    else GS_HIP(hipMemcpy2DAsync(dst, w, src, stride, w, n, hipMemcpyDeviceToHost, c->side));
    GS_HIP(hipEventRecord(c->ev_counts, c->side));
    return GS_OK;
}

// A speculative window is left pending: verified by the next merge_window, or by any call that
// consumes the emission first (cc_settle). (slot, buf): what a tail would be sent from.
int settle_cb(void* ctx);
void leave_pending(gs_comm_t* c, gs_cc_t* h, uint64_t slot, uint32_t* buf) {
    c->pend = {true, slot, buf};
    cc_set_settle(h, settle_cb, c);
}

// Rank 0 of a gather or a tree never exports: its marking goes off once.
int root_stops_marking(gs_comm_t* c, gs_cc_t* h) {
    if (c->root_marking_off) return GS_OK;
    GS_TRY(gs_cc_set_marking(h, 0));
    c->root_marking_off = true;
    return GS_OK;
}

// "Count, then pairs", the exact point-to-point message. Sender: the count word *dcount (device)
// is read by the host (a wait), sent, and then exactly the *n pairs it counts.
int send_counted(gs_comm_t* c, const CcInfo& in, const unsigned long long* dcount, const uint32_t* pairs, int peer,
                 uint64_t* n) {
    const int P = c->world;
    hipStream_t s = in.stream;
    GS_HIP(hipMemcpyAsync(c->hcnt + P, dcount, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    GS_HIP(hipStreamSynchronize(s));
    *n = c->hcnt[P];
    GS_TRY(send(c, dcount, sizeof(unsigned long long), peer, s));
    if (*n) GS_TRY(send(c, pairs, *n * pbytes(in), peer, s));
    c->bytes_sent += *n * pbytes(in);              // (the 8-byte count message is not counted here)
    return GS_OK;
}
// Receiver: the count words of senders [q0, q1) in one group into dcnt[q], then on the host in
// hcnt[q] (a wait) ...
int recv_counts(gs_comm_t* c, int q0, int q1, hipStream_t s) {
    Group g(c);
    for (int q = q0; q < q1; ++q) GS_TRY(recv(c, c->dcnt + q, sizeof(unsigned long long), q, s));
    GS_TRY(g.end());
    GS_HIP(hipMemcpyAsync(c->hcnt, c->dcnt, q1 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    GS_HIP(hipStreamSynchronize(s));
    return GS_OK;
}
// ... and the cnt[q] pairs of every sender q in one group, packed in recvbuf in rank order
// (plan::packed_offsets; grown to the total first).
int recv_packed(gs_comm_t* c, const CcInfo& in, const std::vector<uint64_t>& cnt, std::vector<uint64_t>* off) {
    hipStream_t s = in.stream;
    const uint64_t total = plan::packed_offsets(cnt, off);
    GS_TRY(ensure(c->recvbuf, (size_t)total * pbytes(in), s));
    Group g(c);
    for (size_t q = 0; q < cnt.size(); ++q)
        if (cnt[q]) GS_TRY(recv(c, c->recvbuf + pwords(in) * (*off)[q], cnt[q] * pbytes(in), (int)q, s));
    GS_TRY(g.end());
    c->bytes_recv += total * pbytes(in);
    return GS_OK;
}

int prepare(gs_comm_t* c, gs_cc_t* h, CcInfo* info, int mode) {
    GS_TRY(cc_info(h, info));
    if (mode == GS_MERGE_PREFILTER && info->sparse)
        return fail(GS_ERR_UNSUPPORTED, "GS_MERGE_PREFILTER: dense ids only");
    if (!info->marks && mode != GS_MERGE_PREFILTER)     // (the pre-filter exports no deltas)
        return fail(GS_ERR_UNSUPPORTED, "gs_cc_merge_window: handle created without GS_CC_TRACK_MARKS");
    if (info->device != c->device) return fail(GS_ERR_INVALID, "gs_cc_merge_window: handle on device %d, communicator on %d",
                                               info->device, c->device);
    const uint64_t need = 2ull * info->cap;        // an export never exceeds 2 x capacity pairs
    if (c->cap_pairs < need || c->pair_bytes != pbytes(*info)) {
        c->cap_pairs = 0;
        for (auto* b : {&c->sendbuf, &c->sendbuf2}) {
            b->reset();                            // (a new pair size: new buffers even where the old would do)
            GS_TRY(b->grow((size_t)(need + 1) * pbytes(*info) / 4, "exchange buffers"));      // + a count word
        }
        c->cap_pairs = need;
        c->send_pairs = need + 1;
        c->pair_bytes = pbytes(*info);
    }
    return GS_OK;
}

// GS_MERGE_PREFILTER sender: room for every edge of a slice of m edges to survive (a slice can be
// larger than the 2 x capacity pairs the deltas are sized for). Nothing is pending here (the
// window was settled before merge_prefilter), so the old buffers are free once the stream drains.
int ensure_send(gs_comm_t* c, const CcInfo& in, uint64_t m) {
    if (m + 1 <= c->send_pairs) return GS_OK;
    c->pend.buf = nullptr;
    c->send_pairs = 0;
    const uint64_t want = std::max<uint64_t>(m + 1, c->cap_pairs + 1);
    GS_TRY(c->sendbuf.grow((size_t)want * pwords(in), "prefilter send buffers", in.stream));
    GS_TRY(c->sendbuf2.grow((size_t)want * pwords(in), "prefilter send buffers", in.stream));
    c->send_pairs = want;
    return GS_OK;
}

// ---- GS_MERGE_ALLGATHER: the replicated summary ----

// Folds deltas laid out in slots of m pairs (slot q: cnt[q] real pairs, then copies of its first
// pair; slot `skip` is not folded). While the deltas are big (young windows: components not yet
// joined) each slot is its own fold call, whose short head launch makes the big joins first
// (cc_api.hip kMergeHead); otherwise runs of slots go in one call.
int fold_slots(gs_cc_t* h, const CcInfo& in, const uint32_t* buf, uint64_t m, const std::vector<uint64_t>& cnt, int skip) {
    const int P = (int)cnt.size();
    const uint64_t pw = pwords(in);
    auto folds = [&](int q) { return q != skip && cnt[q] != 0; };
    uint64_t mx = 0;
    for (int q = 0; q < P; ++q) if (folds(q)) mx = std::max(mx, cnt[q]);
    if (mx == 0) return GS_OK;
    if (mx > plan::kBulkDeltaPairs) {
        for (int q = 0; q < P; ++q)
            if (folds(q)) GS_TRY(cc_fold_pairs_any(h, buf + pw * (uint64_t)q * m, cnt[q]));
        return GS_OK;
    }
    int q = 0;
    while (q < P) {
        if (!folds(q)) { ++q; continue; }
        int e = q;
        while (e + 1 < P && folds(e + 1)) ++e;
        const uint64_t npairs = (uint64_t)(e - q) * m + cnt[e];     // the last slot: its real pairs only
        GS_TRY(cc_fold_pairs_any(h, buf + pw * (uint64_t)q * m, npairs));
        q = e + 1;
    }
    return GS_OK;
}

// Every rank's cnt[q] pairs (this rank's at `mine`), padded to slots of m pairs, all-gathered, and
// the other ranks' folded with marking paused: their deltas are theirs to export.
int fold_foreign_slots(gs_comm_t* c, gs_cc_t* h, const CcInfo& in, uint32_t* mine, uint64_t m, const std::vector<uint64_t>& cnt) {
    const int P = c->world;
    hipStream_t s = in.stream;
    const uint64_t n = cnt[c->rank];
    if (n && n < m) pad_pairs(in.sparse, mine, n, m, s);
    GS_HIP(hipGetLastError());
    GS_TRY(ensure(c->recvbuf, (size_t)P * m * pbytes(in), s));
    GS_TRY(allgather(c, mine, c->recvbuf, m * pbytes(in), s));
    GS_TRY(gs_cc_set_marking(h, 0));
    const int rc = fold_slots(h, in, c->recvbuf, m, cnt, c->rank);
    GS_TRY(gs_cc_set_marking(h, in.marking ? 1 : 0));   // the caller's marking state back
    GS_TRY(rc);
    c->bytes_sent += m * pbytes(in) * (P - 1);
    c->bytes_recv += m * pbytes(in) * (P - 1);
    return GS_OK;
}

// One exact window of the replicated summary: counts all-gathered and read by the host, deltas
// padded to the largest count and all-gathered, the others' slots folded, the close. The largest
// delta sizes the next window's speculative slot.
int exchange_exact(gs_comm_t* c, gs_cc_t* h, const CcInfo& in) {
    const int P = c->world;
    hipStream_t s = in.stream;
    GS_TRY(cc_export_async(h, c->sendbuf, c->cap_pairs, c->dcnt + P));
    GS_TRY(allgather(c, c->dcnt + P, c->dcnt, sizeof(unsigned long long), s));
    GS_HIP(hipMemcpyAsync(c->hcnt, c->dcnt, P * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    GS_HIP(hipStreamSynchronize(s));               // the slot size is the largest delta
    std::vector<uint64_t> cnt(c->hcnt.get(), c->hcnt.get() + P);
    const uint64_t maxc = *std::max_element(cnt.begin(), cnt.end());
    if (maxc) GS_TRY(fold_foreign_slots(c, h, in, c->sendbuf, maxc, cnt));
    GS_TRY(gs_cc_close_window(h));
    c->st.spec_slot = plan::next_slot(c->cap_pairs, maxc);
    c->last_delta = maxc;
    return GS_OK;
}

// Replicated global summary: every rank folds the others' deltas, so every rank's giant filter is
// the global one and its next delta holds only connectivity new to the whole job.
// Speculative single-collective round (once a slot size S is known): every rank exports its WHOLE
// delta behind a count word, right after its own fold, and the first S pairs of every rank are
// all-gathered in ONE RCCL call; the others' slots are folded and the window is closed with the
// counts read on the device. The host does NOT wait for the counts here: the window is left
// pending (settle_allgather) and verified at the start of the next merge_window, or by any call
// that consumes the emission first (cc_settle: stats, checksum, emit_*, find, sync, ...), by
// which time the counts are long on the host — so the host can enqueue the next window's fold
// while this window's exchange and close still run. A delta larger than S (every rank sees every
// count, so all agree) has its tail sent in one more all-gather, from the same export: the pairs
// must be the exporter's state right after its own fold — re-exported after folding the others'
// slots (marking paused), a root of its own that a foreign pair hooked would vanish from its
// pairs. A tail folded after the next window's local fold is still exact for every emission a
// caller can observe: the next emission closes after it, and the pending window's own emission is
// only readable through a call that settles first. The first window of a stream runs the exact
// round and sizes S.
int settle_allgather(gs_comm_t* c, bool close) {
    if (!c->pend.open) return GS_OK;
    c->pend.open = false;
    gs_cc_t* h = c->bound;
    CcInfo in;
    GS_TRY(cc_info(h, &in));
    DeviceGuard g(in.device);
    const int P = c->world;
    const uint64_t S = c->pend.slot;
    GS_HIP(hipEventSynchronize(c->ev_counts));      // normally complete long ago
    std::vector<uint64_t> tail(P, 0);
    uint64_t folded = 0, mt = 0, maxc = 0;
    for (int q = 0; q < P; ++q) {
        const uint64_t n = c->hcnt[q];
        if (n > c->cap_pairs - 1) return fail(GS_ERR_CAPACITY, "rank %d delta of %llu pairs past the export buffer", q,
                                              (unsigned long long)n);
        maxc = std::max<uint64_t>(maxc, n);
        tail[q] = plan::tail_of(n, S);
        mt = std::max<uint64_t>(mt, tail[q]);
        if (q != c->rank) folded += n;
    }
    cc_count_folded(h, folded);
    if (mt) {                                                   // tails past S: one more all-gather
        ++c->overflows;
        GS_TRY(fold_foreign_slots(c, h, in, c->pend.buf + 2 + pwords(in) * S, mt, tail));   // this rank's pairs [S, n)
        if (close) GS_TRY(gs_cc_close_window(h));              // (from merge_window: its close follows)
    }
    c->st.spec_slot = plan::next_slot(c->cap_pairs, maxc);
    c->last_delta = maxc;
    return GS_OK;
}

int merge_allgather(gs_comm_t* c, gs_cc_t* h, const CcInfo& in) {
    const int P = c->world;
    hipStream_t s = in.stream;
    if (c->st.spec_slot == 0 && !c->pend.open) return exchange_exact(c, h, in);
    // 1. this window's export, into the buffer the pending window does not use: its roots are
    //    this rank's forest right after its own fold (the pending window's tails, foreign pairs
    //    folded with marking paused, must not be under them: a root of its own they hooked would
    //    vanish from its pairs)
    uint32_t* send = (c->pend.open && c->pend.buf == c->sendbuf) ? c->sendbuf2 : c->sendbuf;
    GS_TRY(cc_export_async(h, send + 2, c->cap_pairs - 1, reinterpret_cast<unsigned long long*>(send), 2 * c->last_delta));
    // 2. the previous window's verification (its tail round, if any, is the next collective on
    //    every rank); it sizes this window's slot
    if (c->pend.open) {
        cc_set_settle(h, nullptr, nullptr);
        GS_TRY(settle_allgather(c, false));
    }
    const uint64_t S = c->st.spec_slot;
    const uint64_t slot_words = plan::slot_words(S, pbytes(in));   // [u64 count][S pairs]
    GS_TRY(ensure(c->slotbuf, (size_t)P * slot_words * 4, s));
    GS_TRY(allgather(c, send, c->slotbuf, slot_words * 4, s));
    GS_TRY(counts_aside(c, c->slotbuf, slot_words * 4, P, c->hcnt, s));
    GS_TRY(cc_fold_slots(h, c->slotbuf, slot_words, P, c->rank, S));
    GS_TRY(gs_cc_close_window(h));                              // optimistic: no delta exceeded S
    c->bytes_sent += slot_words * 4 * (P - 1);
    c->bytes_recv += slot_words * 4 * (P - 1);
    leave_pending(c, h, S, send);
    return GS_OK;
}

// ---- the gather to rank 0 (the Merger): GS_MERGE_GATHER's deltas, GS_MERGE_PREFILTER's survivors ----
// windowAll: every other rank sends what its window produced straight to rank 0, which folds it
// all, closes and emits.
// An exact round (the first window of a stream, and the others plan::exact_round names): the count
// is sent first and read by the host on both sides, then exactly the pairs. It sizes every
// sender's speculative slot (gslot).
// A speculative round: each sender sends [count | S_q pairs] in ONE message, S_q sized from its
// own last count; rank 0 receives every slot, folds them with the counts read on the device and
// closes — no host wait on either side. The window is left pending and verified lazily by
// settle_gather, as the all-gather's is.
// Either way each side sizes the sender's next slot from the same count (size_slot), so both agree
// without another message.
struct GatherKind {
    bool survivors;          // a sender's pairs are cc_filter_async's survivors of its slice (it has no forest),
                             // not cc_export_async's delta
    bool young_exact;        // the first plan::kExactYoung windows are exact rounds
    bool fold_per_sender;    // rank 0 folds big exact deltas (> plan::kBulkDeltaPairs) one call per sender; else
                             // always one call (one per slice cost ~7 dependent launches per young window)
    bool root_checks_cap;    // rank 0 refuses a count past the export buffer (survivors are bounded by the
                             // sender's slice, which its own buffers hold)
    bool sender_closes;      // the sender closes its own summary (its giant filter)
    bool counts_count_word;  // the byte counters include an exact round's 8-byte count messages (rank 0: when
                             // a survivor arrived); bench lines are compared across rounds, so this stays
};
constexpr GatherKind kGatherDeltas{false, false, true, true, true, false};
constexpr GatherKind kGatherSurvivors{true, true, false, false, false, true};
const GatherKind& gather_kind(const gs_comm_t* c) { return c->mode == GS_MERGE_PREFILTER ? kGatherSurvivors : kGatherDeltas; }

// GSGPU_PREFILTER_LOG=1: a sender's survivor count per window on stderr (once known: at once in
// the exact rounds, at the settle of a speculative one) — the real staleness of the broadcast
// bitmap, which tools/sim_ranks.py's filter against the Merger's current state cannot show
void log_survivors(const gs_comm_t* c, uint64_t n) {
    static const bool on = [] { const char* e = getenv("GSGPU_PREFILTER_LOG"); return e && atoi(e) != 0; }();
    if (on) fprintf(stderr, "[gsgpu prefilter] rank %d survivors %llu\n", c->rank, (unsigned long long)n);
}

// sender q's count n is known (on q and on rank 0 alike): its next slot
void size_slot(gs_comm_t* c, int q, uint64_t n) { c->st.gslot[q] = plan::next_slot(c->cap_pairs, n); }

// One window's round. (a, b, m): a survivors sender's slice; win: the window's number in the stream.
int gather_round(gs_comm_t* c, gs_cc_t* h, const CcInfo& in, const GatherKind& k, const void* a, const void* b, uint64_t m,
                 uint64_t win) {
    const int P = c->world;
    hipStream_t s = in.stream;
    const bool exact = plan::exact_round(k.young_exact, win, !c->st.gslot.empty(), P, kMaxSlotCaps);
    if (c->st.gslot.empty()) c->st.gslot.assign(P, 0);
    if (c->rank != 0) {
        // [count word | pairs] into the send buffer the last window's tail does not use (an exact
        // round: the first; an exact delta export has its count in dcnt[P], no count word in front)
        uint32_t* buf = (!exact && c->pend.buf == c->sendbuf) ? c->sendbuf2 : c->sendbuf;
        unsigned long long* dcount = reinterpret_cast<unsigned long long*>(buf);
        const uint32_t* pairs = buf + 2;
        if (k.survivors) {
            GS_TRY(cc_filter_async(h, a, b, m, buf + 2, c->send_pairs - 1, dcount));
        } else if (exact) {
            dcount = c->dcnt + P;
            pairs = buf;
            GS_TRY(cc_export_async(h, buf, c->cap_pairs, dcount));
        } else {
            GS_TRY(cc_export_async(h, buf + 2, c->cap_pairs - 1, dcount, 2 * c->last_delta));
        }
        const uint64_t S = c->st.gslot[c->rank];
        if (exact) {
            uint64_t n = 0;
            GS_TRY(send_counted(c, in, dcount, pairs, 0, &n));
            if (k.counts_count_word) c->bytes_sent += 8;
            size_slot(c, c->rank, n);
            c->last_delta = n;
            if (k.survivors) {
                c->pend.buf = buf;
                log_survivors(c, n);
            }
        } else {
            GS_TRY(send(c, buf, plan::slot_bytes(S, pbytes(in)), 0, s));
            GS_TRY(counts_aside(c, buf, 0, 1, c->hcnt + P, s));
            c->bytes_sent += plan::slot_bytes(S, pbytes(in));
        }
        if (k.sender_closes) GS_TRY(gs_cc_close_window(h));
        if (!exact) leave_pending(c, h, S, buf);   // (after the close: a close settles what is pending)
        return GS_OK;
    }
    GS_TRY(root_stops_marking(c, h));
    if (exact) {
        GS_TRY(recv_counts(c, 1, P, s));
        std::vector<uint64_t> cnt(P, 0), off;
        uint64_t mx = 0;
        for (int q = 1; q < P; ++q) {
            cnt[q] = c->hcnt[q];
            mx = std::max(mx, cnt[q]);
            size_slot(c, q, cnt[q]);
        }
        if (mx) {
            GS_TRY(recv_packed(c, in, cnt, &off));
            if (k.fold_per_sender && mx > plan::kBulkDeltaPairs) {   // (head launch first)
                for (int q = 1; q < P; ++q)
                    if (cnt[q]) GS_TRY(cc_fold_pairs_any(h, c->recvbuf + pwords(in) * off[q], cnt[q]));
            } else {
                GS_TRY(cc_fold_pairs_any(h, c->recvbuf, off.back()));
            }
            if (k.counts_count_word) c->bytes_recv += 8 * (P - 1);
        }
        c->last_delta = mx;
        return gs_cc_close_window(h);
    }
    uint64_t smax = 0;
    for (int q = 1; q < P; ++q) smax = std::max(smax, c->st.gslot[q]);
    const uint64_t slot_words = plan::slot_words(smax, pbytes(in));
    GS_TRY(ensure(c->slotbuf, (size_t)P * slot_words * 4, s));
    {
        Group g(c);
        for (int q = 1; q < P; ++q)
            GS_TRY(recv(c, c->slotbuf + (uint64_t)q * slot_words, plan::slot_bytes(c->st.gslot[q], pbytes(in)), q, s));
        GS_TRY(g.end());
    }
    GS_TRY(counts_aside(c, c->slotbuf, slot_words * 4, P, c->hcnt, s));
    GS_TRY(cc_fold_slots(h, c->slotbuf, slot_words, P, 0, smax, c->st.gslot.data()));
    GS_TRY(gs_cc_close_window(h));                              // optimistic: no sender outgrew its slot
    for (int q = 1; q < P; ++q) c->bytes_recv += plan::slot_bytes(c->st.gslot[q], pbytes(in));
    leave_pending(c, h, 0, nullptr);                            // (rank 0 sends no tail)
    return GS_OK;
}

// The speculative gather's verification (as settle_allgather): a sender whose count outgrew its
// slot sends the tail [S, n) from the same buffer; rank 0 knows which senders overflowed from the
// count words of their slots (on the host by now), receives those tails, folds them and, when
// called from cc_settle (an emission read), closes again.
int settle_gather(gs_comm_t* c, bool close) {
    if (!c->pend.open) return GS_OK;
    c->pend.open = false;
    gs_cc_t* h = c->bound;
    const GatherKind& k = gather_kind(c);
    CcInfo in;
    GS_TRY(cc_info(h, &in));
    DeviceGuard g(in.device);
    const int P = c->world;
    GS_HIP(hipEventSynchronize(c->ev_counts));      // normally complete long ago
    if (c->rank != 0) {
        const uint64_t n = c->hcnt[P], S = c->pend.slot;
        if (n > c->send_pairs - 1) return fail(GS_ERR_CAPACITY, "delta of %llu pairs past the export buffer", (unsigned long long)n);
        if (const uint64_t t = plan::tail_of(n, S)) {
            ++c->overflows;
            GS_TRY(send(c, c->pend.buf + 2 + pwords(in) * S, t * pbytes(in), 0, in.stream));
            c->bytes_sent += t * pbytes(in);
        }
        size_slot(c, c->rank, n);
        c->last_delta = n;
        if (k.survivors) log_survivors(c, n);
        return GS_OK;
    }
    std::vector<uint64_t> tail(P, 0), off;
    uint64_t mt = 0, mx = 0, folded = 0;
    for (int q = 1; q < P; ++q) {
        const uint64_t n = c->hcnt[q];
        if (k.root_checks_cap && n > c->cap_pairs - 1)
            return fail(GS_ERR_CAPACITY, "rank %d delta of %llu pairs past the export buffer", q, (unsigned long long)n);
        tail[q] = plan::tail_of(n, c->st.gslot[q]);
        folded += n - tail[q];
        mt = std::max(mt, tail[q]);
        mx = std::max(mx, n);
        size_slot(c, q, n);
    }
    cc_count_folded(h, folded);
    c->last_delta = mx;
    if (mt) {
        ++c->overflows;
        GS_TRY(recv_packed(c, in, tail, &off));
        GS_TRY(cc_fold_pairs_any(h, c->recvbuf, off.back()));
        if (close) GS_TRY(gs_cc_close_window(h));
    }
    return GS_OK;
}

int abort_exchange(gs_comm_t* c, int rc);

// cc_settle's callback: a failed verification fails the group (peers may be in the tail round)
int settle_cb(void* ctx) {
    gs_comm_t* c = static_cast<gs_comm_t*>(ctx);
    const int rc = (c->mode == GS_MERGE_GATHER || c->mode == GS_MERGE_PREFILTER) ? settle_gather(c, true)
                                                                                 : settle_allgather(c, true);
    return rc == GS_OK ? rc : abort_exchange(c, rc);
}

int merge_gather(gs_comm_t* c, gs_cc_t* h, const CcInfo& in) {
    return gather_round(c, h, in, kGatherDeltas, nullptr, nullptr, 0, 0);
}

// ---- GS_MERGE_PREFILTER: the partitions filter, the Merger unions ----
// SummaryBulkAggregation.java:76-83: every partition folds its slice of a window (UpdateCC) and the
// window's partials go to the parallelism-1 Merger, which combines them and emits. Here ranks
// 1..P-1 keep no forest: a rank runs only the giant FILTER of the fold over its slice, against the
// giant bitmap and root rank 0 broadcasts (a stale bitmap is safe: components only merge until
// reset), with its own LDS hot / L2 warm sets, and sends the survivors — plain (u, v) edges — to
// rank 0 in the gather's round (gather_round, kGatherSurvivors). Rank 0 folds its own slice and
// every rank's survivors, closes and emits. The filter (the fold's expensive, read-only part) runs
// on P - 1 GPUs in parallel; the unions, the close and the emission stay on the Merger, whose
// per-window work is the survivors (~3.5 % of a steady RMAT-26 window) instead of every rank's full
// delta fold. The bitmap and the giant words go out after rank 0's closes on the schedule in
// exchange_plan.hpp (bcast_sync, bcast_async): rank 0 snapshots [gbits | giant words] right after
// the close and broadcasts the snapshot on a side stream over a communicator of their own, while
// it folds the next windows; a sender receives into one of two staging slots on its side stream
// and installs the state before its filter kBcastLag windows later. A rank may fold no slice of its
// own (n == 0): every rank still runs every window's exchange (the window count is agreed per call,
// gs_cc_fold_windows).

// side stream, events and staging of the asynchronous broadcasts (first use)
int bside_init(gs_comm_t* c, uint64_t slot_words) {
    if (c->bc.bstage) return GS_OK;
    GS_TRY(make_whole(c->bc, (size_t)slot_words * (c->rank == 0 ? 1 : 2)));
    c->bslot_words = slot_words;
    return GS_OK;
}

// rank 0, after close(win): the snapshot and its broadcast, off the handle's stream
int bcast_async_send(gs_comm_t* c, gs_cc_t* h, hipStream_t s) {
    uint32_t *gb = nullptr, *words = nullptr;
    uint64_t gbytes = 0;
    GS_TRY(cc_filter_state(h, &gb, &gbytes, &words));
    GS_TRY(bside_init(c, gbytes / 4 + 2));
    // the snapshot is taken on the handle's stream, right after the close: a copy on the side stream
    // could overlap the next close, and a giant switch there (the bitmap rebuilt for another
    // component) would mix two components' bits (8 MiB at 2^26 ids: a few us). The previous
    // broadcast must have read the buffer first.
    GS_HIP(hipStreamWaitEvent(s, c->bc.ev_bmain, 0));
    GS_HIP(hipMemcpyAsync(c->bc.bstage, gb, gbytes, hipMemcpyDeviceToDevice, s));
    GS_HIP(hipMemcpyAsync(c->bc.bstage + gbytes / 4, words, 2 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    GS_HIP(hipEventRecord(c->bc.ev_brecv[0], s));                  // the snapshot is complete
    GS_HIP(hipStreamWaitEvent(c->bc.bside, c->bc.ev_brecv[0], 0));
    GS_TRY(bcast(c, c->bc.bstage, gbytes + 8, c->bc.bside, true));
    GS_HIP(hipEventRecord(c->bc.ev_bmain, c->bc.bside));              // the buffer may be rewritten after this
    c->bytes_sent += (gbytes + 8) * (c->world - 1);
    return GS_OK;
}

// sender, in the call of window win: receive the state rank 0 broadcasts after close(win) into a slot
int bcast_async_recv(gs_comm_t* c, gs_cc_t* h, uint64_t win) {
    uint32_t *gb = nullptr, *words = nullptr;
    uint64_t gbytes = 0;
    GS_TRY(cc_filter_state(h, &gb, &gbytes, &words));
    GS_TRY(bside_init(c, gbytes / 4 + 2));
    const int k = plan::bcast_slot(win);
    // (the slot's last install was recorded in ev_bmain, which the side stream waits for)
    GS_HIP(hipStreamWaitEvent(c->bc.bside, c->bc.ev_bmain, 0));
    GS_TRY(bcast(c, c->bc.bstage + (size_t)k * c->bslot_words, gbytes + 8, c->bc.bside, true));
    GS_HIP(hipEventRecord(c->bc.ev_brecv[k], c->bc.bside));
    c->st.bpend[k] = (int64_t)win;
    c->bytes_recv += gbytes + 8;
    return GS_OK;
}

// sender, before the filter of window win: install the state of window win - kBcastLag if it was sent
int bcast_async_install(gs_comm_t* c, gs_cc_t* h, uint64_t win, hipStream_t s) {
    uint64_t j = 0;
    if (!plan::bcast_install_due(win, &j)) return GS_OK;
    const int k = plan::bcast_slot(j);
    if (c->st.bpend[k] != (int64_t)j) return GS_OK;
    uint32_t *gb = nullptr, *words = nullptr;
    uint64_t gbytes = 0;
    GS_TRY(cc_filter_state(h, &gb, &gbytes, &words));
    const uint32_t* slot = c->bc.bstage + (size_t)k * c->bslot_words;
    GS_HIP(hipStreamWaitEvent(s, c->bc.ev_brecv[k], 0));
    GS_HIP(hipMemcpyAsync(gb, slot, gbytes, hipMemcpyDeviceToDevice, s));
    GS_TRY(cc_install_giant(h, slot + gbytes / 4));
    GS_HIP(hipEventRecord(c->bc.ev_bmain, s));                      // slot k free for the next receive
    c->st.bpend[k] = -1;
    return GS_OK;
}

int bcast_filter_state(gs_comm_t* c, gs_cc_t* h, hipStream_t s) {
    uint32_t *gb = nullptr, *words = nullptr;
    uint64_t gbytes = 0;
    GS_TRY(cc_filter_state(h, &gb, &gbytes, &words));
    GS_TRY(c->bword.grow(2, "broadcast words"));
    if (c->rank == 0) GS_HIP(hipMemcpyAsync(c->bword, words, 2 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    {
        Group g(c);
        GS_TRY(bcast(c, gb, gbytes, s));
        GS_TRY(bcast(c, c->bword, 2 * sizeof(uint32_t), s));
        GS_TRY(g.end());
    }
    if (c->rank != 0) GS_TRY(cc_install_giant(h, c->bword));
    if (c->rank == 0) c->bytes_sent += (gbytes + 8) * (c->world - 1);
    else c->bytes_recv += gbytes + 8;
    return GS_OK;
}

int merge_prefilter(gs_comm_t* c, gs_cc_t* h, const CcInfo& in, const void* a, const void* b, uint64_t m) {
    hipStream_t s = in.stream;
    const uint64_t win = c->st.win++;
    if (c->rank != 0) {
        GS_TRY(ensure_send(c, in, m));
        GS_TRY(bcast_async_install(c, h, win, s));
    }
    GS_TRY(gather_round(c, h, in, kGatherSurvivors, a, b, m, win));
    if (plan::bcast_sync(win)) GS_TRY(bcast_filter_state(c, h, s));
    if (plan::bcast_async(win)) GS_TRY(c->rank == 0 ? bcast_async_send(c, h, s) : bcast_async_recv(c, h, win));
    return GS_OK;
}

// ---- GS_MERGE_TREE ----
// ConnectedComponentsTree's pairwise rounds (SummaryTreeReduce.enhance; plan::tree_role): a
// receiver folds its sender's delta with marking on (it forwards what it gained in a later round).
// Every round is exact, with its host wait.
int merge_tree(gs_comm_t* c, gs_cc_t* h, const CcInfo& in) {
    const int P = c->world;
    if (c->rank == 0) GS_TRY(root_stops_marking(c, h));
    for (int step = 1; step < P; step *= 2) {
        const plan::TreeRole role = plan::tree_role(c->rank, P, step);
        if (role.kind == plan::TreeRole::Send) {   // done for this window after this
            uint64_t n = 0;
            GS_TRY(cc_export_async(h, c->sendbuf, c->cap_pairs, c->dcnt + P));
            GS_TRY(send_counted(c, in, c->dcnt + P, c->sendbuf, role.peer, &n));
            break;
        }
        if (role.kind == plan::TreeRole::Recv) {
            GS_TRY(recv_counts(c, role.peer, role.peer + 1, in.stream));
            std::vector<uint64_t> cnt(P, 0), off;
            cnt[role.peer] = c->hcnt[role.peer];
            if (cnt[role.peer]) {
                GS_TRY(recv_packed(c, in, cnt, &off));
                GS_TRY(cc_fold_pairs_any(h, c->recvbuf, cnt[role.peer]));
            }
        }
    }
    return gs_cc_close_window(h);
}

int alloc_common(gs_comm_t* c, int rank, int world, int device) {
    c->rank = rank;
    c->world = world;
    c->device = device;
    for (Event* e : {&c->ev_ready, &c->ev_counts, &c->ev_done, &c->ev_slots}) GS_TRY(e->create());
    GS_TRY(c->side.create());
    GS_TRY(c->dcnt.grow(c->world + 1, "communicator scratch"));
    GS_TRY(c->hcnt.alloc(c->world + 1, "communicator scratch"));
    GS_HIP(hipMemset(c->dcnt, 0, (c->world + 1) * sizeof(unsigned long long)));
    return GS_OK;
}

}  // namespace

extern "C" {

int gs_comm_unique_id(void* id, uint64_t id_bytes) {
    if (!id || id_bytes < sizeof(ncclUniqueId)) return fail(GS_ERR_INVALID, "gs_comm_unique_id: need %zu bytes", sizeof(ncclUniqueId));
    ncclUniqueId u;
    GS_NCCL(ncclGetUniqueId(&u));
    memcpy(id, &u, sizeof(u));
    return GS_OK;
}

int gs_comm_create(gs_comm_t** out, const void* unique_id, int rank, int world, int device) {
    if (!out || !unique_id) return fail(GS_ERR_INVALID, "gs_comm_create: null argument");
    *out = nullptr;
    if (world < 1 || rank < 0 || rank >= world) return fail(GS_ERR_INVALID, "gs_comm_create: rank %d of %d", rank, world);
    DeviceGuard g(device);
    if (!g.ok) return fail(GS_ERR_HIP, "gs_comm_create: hipSetDevice(%d) failed", device);
    std::unique_ptr<gs_comm_t> c(new gs_comm_t());
    GS_TRY(alloc_common(c.get(), rank, world, device));
    ncclUniqueId u;
    memcpy(&u, unique_id, sizeof(u));
    const ncclResult_t r = ncclCommInitRank(&c->nccl, world, u, rank);
    if (r != ncclSuccess) {
        c->nccl = nullptr;
        const int rc = nccl_fail(r, "ncclCommInitRank");
        gs_comm_destroy(c.release());
        return rc;
    }
    *out = c.release();
    return GS_OK;
}

int gs_comm_create_local(gs_comm_t** comms, int world, int device) {
    if (!comms || world < 1) return fail(GS_ERR_INVALID, "gs_comm_create_local: bad arguments");
    DeviceGuard g(device);
    if (!g.ok) return fail(GS_ERR_HIP, "gs_comm_create_local: hipSetDevice(%d) failed", device);
    auto grp = std::make_shared<LocalGroup>(world);
    for (int r = 0; r < world; ++r) comms[r] = nullptr;
    for (int r = 0; r < world; ++r) {
        gs_comm_t* c = new gs_comm_t();
        c->local = grp;
        comms[r] = c;
        const int rc = alloc_common(c, r, world, device);
        if (rc != GS_OK) {
            for (int q = 0; q <= r; ++q) { gs_comm_destroy(comms[q]); comms[q] = nullptr; }
            return rc;
        }
    }
    return GS_OK;
}

int gs_comm_destroy(gs_comm_t* c) {
    if (!c) return GS_OK;
    DeviceGuard g(c->device);
    if (c->pend.open && c->bound) {                 // verify the last window (peers may be in its tail
        cc_set_settle(c->bound, nullptr, nullptr);  // round), then the handle forgets this communicator
        if (!c->broken) (void)settle_cb(c);
    }
    (void)hipDeviceSynchronize();
    if (c->nccl_side) (void)ncclCommDestroy(c->nccl_side);
    if (c->nccl) (void)ncclCommDestroy(c->nccl);
    delete c;                                       // the owners free what it holds (owned.hpp)
    return GS_OK;
}

int gs_comm_info(gs_comm_t* c, int* rank, int* world, uint64_t* bytes_sent, uint64_t* bytes_recv, uint64_t* exchanges,
                 uint64_t* overflows) {
    if (!c) return fail(GS_ERR_INVALID, "null communicator");
    // (a pending window's overflow round is counted when it is verified: the next merge_window or
    // any call that consumes the emission)
    if (overflows) *overflows = c->overflows;
    if (rank) *rank = c->rank;
    if (world) *world = c->world;
    if (bytes_sent) *bytes_sent = c->bytes_sent;
    if (bytes_recv) *bytes_recv = c->bytes_recv;
    if (exchanges) *exchanges = c->exchanges;
    return GS_OK;
}

namespace {
// A rank that fails inside an exchange would leave its peers blocked in the next collective: tear
// the communicator down so they fail too (RCCL: ncclCommAbort; in-process: wake every waiter).
int abort_exchange(gs_comm_t* c, int rc) {
    const std::string msg = last_error();
    c->broken = true;
    if (c->nccl_side) {
        (void)ncclCommAbort(c->nccl_side);
        c->nccl_side = nullptr;
    }
    if (c->nccl) {
        (void)ncclCommAbort(c->nccl);
        c->nccl = nullptr;
    }
    if (c->local) c->local->fail_all();
    last_error() = msg;
    return rc;
}

int merge_window(gs_cc_t* h, gs_comm_t* c, int mode, const void* a, const void* b, uint64_t m) {
    CcInfo in;
    GS_TRY(prepare(c, h, &in, mode));
    // a communicator carries per-stream state (the speculative slot sizes, rank 0's paused
    // marking): it serves one handle in one mode; a reset of that handle starts a new stream
    if (c->bound && (c->bound != h || c->mode != mode))
        return fail(GS_ERR_INVALID, "gs_cc_merge_window: this communicator serves another handle or mode "
                                    "(one communicator per summary and mode)");
    if (!c->bound) {
        // every rank sizes its exchange buffers from its own handle, and the speculative slots are
        // sized from them on the sending and the receiving side alike (plan::next_slot): agree once,
        // when the communicator is bound, that every rank's capacity and pair width are the same
        // (every rank sees every word, so all fail together on a mismatch)
        const unsigned long long mine = (unsigned long long)c->cap_pairs << 8 | c->pair_bytes;
        GS_TRY(allgather_word(c, mine, in.stream));
        for (int q = 0; q < c->world; ++q)
            if (c->hcnt[q] != mine)
                return fail(GS_ERR_INVALID, "gs_cc_merge_window: rank %d's summary has %llu-pair / %llu-byte exchange "
                            "buffers, rank %d's %llu / %llu: every rank needs the same vertex capacity and id mode",
                            q, c->hcnt[q] >> 8, c->hcnt[q] & 0xFF, c->rank, (unsigned long long)c->cap_pairs,
                            (unsigned long long)c->pair_bytes);
        if (mode == GS_MERGE_PREFILTER && c->nccl && !c->nccl_side)   // (collective: every rank binds here)
            GS_NCCL(ncclCommSplit(c->nccl, 0, c->rank, &c->nccl_side, nullptr));
        c->bound = h;
        c->mode = mode;
        c->reset_gen = in.reset_gen;
    }
    if (mode != GS_MERGE_ALLGATHER) GS_TRY(cc_settle(h));   // (allgather settles after its export)
    if (in.reset_gen != c->reset_gen) {              // the handle was reset: a new stream, whose first
        c->reset_gen = in.reset_gen;                 // window runs the exact round again
        c->st = gs_comm::StreamState();
    }
    DeviceGuard g(in.device);
    switch (mode) {
    case GS_MERGE_ALLGATHER: return merge_allgather(c, h, in);
    case GS_MERGE_GATHER: return merge_gather(c, h, in);
    case GS_MERGE_PREFILTER: return merge_prefilter(c, h, in, a, b, m);
    default: return merge_tree(c, h, in);
    }
}

// The one way into a window's exchange. args: the caller's own argument check (GS_OK, or the
// failure it recorded). Any failure on one rank (a bad argument included) fails the whole group:
// its peers are (or will be) waiting for this rank in a collective.
int enter_exchange(const char* who, int args, gs_cc_t* h, gs_comm_t* c, int mode, const void* a, const void* b, uint64_t m) {
    if (!c) return fail(GS_ERR_INVALID, "%snull communicator", who);
    if (c->broken) return fail(GS_ERR_COMM, "%sthe communicator failed in an earlier exchange", who);
    const int rc = args != GS_OK ? args : merge_window(h, c, mode, a, b, m);
    if (rc != GS_OK) return abort_exchange(c, rc);
    ++c->exchanges;
    return rc;
}
}  // namespace

extern "C++" {
namespace gsgpu {
int cc_comm_rank(const gs_comm_t* c) { return c ? c->rank : 0; }

// GS_MERGE_PREFILTER (gs_cc_fold_windows): every window is an exchange with rank 0, so every rank
// must run the same number of them. Each rank's slice of a short last global window may be empty,
// a rank's whole slice may be empty: the ranks agree on the largest window count (one all-gather of
// a word per call) and a rank past its own edges runs empty windows (a rank with n == 0
// used to skip the exchange and leave its peers waiting in it).
int cc_agree_windows(gs_cc_t* h, gs_comm_t* c, uint64_t mine, uint64_t* most) {
    if (!c) return fail(GS_ERR_INVALID, "null communicator");
    if (c->broken) return fail(GS_ERR_COMM, "the communicator failed in an earlier exchange");
    CcInfo in;
    GS_TRY(cc_info(h, &in));
    GS_TRY(cc_settle(h));                            // (nothing is pending between calls: settled at their end)
    DeviceGuard g(in.device);
    const int rc = allgather_word(c, mine, in.stream);
    if (rc != GS_OK) return abort_exchange(c, rc);
    *most = *std::max_element(c->hcnt.get(), c->hcnt.get() + c->world);
    return GS_OK;
}

// gs_cc_fold_windows with GS_MERGE_PREFILTER: the window's own edges go to the exchange (rank 0
// has folded them already; the other ranks filter them there)
int cc_merge_edges(gs_cc_t* h, gs_comm_t* c, int mode, const void* a, const void* b, uint64_t m) {
    return enter_exchange("", GS_OK, h, c, mode, a, b, m);
}
}  // namespace gsgpu
}  // extern "C++"

int gs_cc_merge_window(gs_cc_t* h, gs_comm_t* c, int mode) {
    int args = GS_OK;
    if (!h) args = fail(GS_ERR_INVALID, "gs_cc_merge_window: null handle");
    else if (mode == GS_MERGE_PREFILTER)
        args = fail(GS_ERR_INVALID, "gs_cc_merge_window: GS_MERGE_PREFILTER needs the window's edges (gs_cc_fold_windows)");
    else if (mode != GS_MERGE_ALLGATHER && mode != GS_MERGE_GATHER && mode != GS_MERGE_TREE)
        args = fail(GS_ERR_INVALID, "gs_cc_merge_window: mode %d", mode);
    return enter_exchange("gs_cc_merge_window: ", args, h, c, mode, nullptr, nullptr, 0);
}

}  // extern "C"
