// deg.hip — streaming vertex degrees and the degree distribution, with edge deletions, on the
// device: the reference's SimpleEdgeStream.getDegrees / getInDegrees / getOutDegrees
// (SimpleEdgeStream.java:413-478) and example/DegreeDistribution.java (:70-132), extern "C" in
// include/gsgpu.h (gs_deg_*).
//
// A vertex event (v, +1 | -1) is the step x -> max(x + change, 0) on v's degree (absent = 0;
// VertexDegreeCounts.flatMap, DegreeDistribution.java:88-110). A run of steps is a function
// x -> max(x + a, b); (a1, b1) then (a2, b2) is (a1 + a2, max(b1 + a2, b2)): associative, not
// commutative. A vertex's degree after a window is max(old + A, B) for the ordered composition
// (A, B) of its events of the window. If the window's deletions at v number at most old, no prefix
// can clamp and new = old + plus - minus; a vertex that fails this test is "at risk".
//
// A window runs on the handle's stream:
//   begin     per-window control words; the sparse distribution table is rebuilt when stale keys
//             fill half of it (one workgroup)
//   count     (GS_DEG_COUNT) one 64-bit atomic add per vertex event on the vertex's accumulator
//             word (low half additions, high half deletions). A workgroup first combines the events
//             of a tile in an LDS table keyed by vertex (an RMAT hub collects thousands of events of
//             a window: one global atomic per workgroup tile instead of one per event); an event
//             whose LDS slot another vertex holds goes to the global word directly. The add that
//             returns 0 puts the vertex on the touched list (one counter add per wave).
//   close     walks the touched list: clears the accumulator, applies the plain sum where the vertex
//             is not at risk, else sets its bit in the at-risk bitmap and leaves its degree alone.
//   exact     only when the close found at-risk vertices (one small read of their event count; never
//             for a window without deletions): the window's vertex events at those vertices become
//             keys vertex | position | sign, are radix-sorted (hipcub, over the bits in use), turned
//             into (head, a, b) elements and inclusive-scanned with the segmented composition; the
//             last element of a vertex's run holds its (A, B). By default (and with
//             GS_DEG_SORT_ALL) every vertex event goes this way instead of being counted (no
//             accumulators, no read): measured faster on every stream of tools/bench_degrees.py.
//   finish    maximum degree (rescanned from the distribution only when a vertex that held the
//             maximum lost degree), the window's statistics into the call's result array.
// Applying a degree change updates degree[], the window's delta list, count[old] / count[new]
// (degrees below kLdsDeg per workgroup in LDS, flushed once; the rest by global atomics into the
// dense array or the sparse table), the checksum and the vertex count. degree[] is written only
// there, and every applying kernel does nothing once an id outside the capacity was seen, so a
// failed window leaves the summary as it was.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <memory>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "owned.hpp"

namespace gsgpu {

constexpr uint32_t kDegThreads = 256;
constexpr uint32_t kDegEPT = 4;                          // events per thread and tile in k_deg_count
constexpr uint32_t kDegTile = kDegThreads * kDegEPT;     // events of a tile
constexpr uint32_t kDegSlots = 2048;                     // LDS slots of a tile (at most 2 x kDegTile vertex events)
constexpr uint32_t kLdsDeg = 1024;                       // degrees counted per workgroup in LDS (RMAT, edge factor 16: most vertices)
constexpr unsigned kDegMaxBlocks = 2048;
constexpr uint32_t kDegDefaultDense = 1u << 16;
constexpr uint32_t kDegMaxTable = 1u << 20;              // slots of the sparse (degree, count) table
constexpr uint32_t kGcThreads = 1024;

struct DegCtl {
    // per window (k_deg_begin)
    uint32_t n_touched, n_delta, n_risk, n_risk_events, n_keys, dirty, m0, newmax, scanmax;
    // per call
    uint32_t range, overflow;
    // the summary
    uint32_t maxdeg, cur, used;
    // restore's validation / emission counters
    uint32_t bad_zero, bad_dup, vmax, n_emit;
    unsigned long long n_vertices, n_degrees, checksum, vsum;
};

struct DegEl {                                           // a run of steps x -> max(x + a, b); head: first of its vertex
    int32_t a, b;
    uint32_t head, pad;
};

// Segmented composition, left operand first in stream order. Associative (a segmented scan
// operator over an associative one), NOT commutative.
struct DegOp {
    __host__ __device__ __forceinline__ DegEl operator()(const DegEl& l, const DegEl& r) const {
        if (r.head) return r;
        DegEl o;
        o.a = l.a + r.a;
        o.b = l.b + r.a > r.b ? l.b + r.a : r.b;
        o.head = l.head;
        o.pad = 0;
        return o;
    }
};

struct DegArgs {
    DegCtl* ctl;
    uint32_t* degree;                 // [cap]
    unsigned long long* acc;          // [cap] window accumulator: low half additions, high half deletions
    uint32_t* touched;                // [cap]
    uint32_t* bits;                   // [cap / 32] at-risk bitmap (zero between windows)
    uint32_t* dv;                     // [cap] the window's degree delta: vertex
    uint32_t* dd;                     //       and its new degree
    unsigned long long* dense;        // [D] count[d], d < D
    unsigned long long* sdense;       // [D] its copy from before the last window (distribution delta)
    uint32_t* tkeys;                  // [3 x tcap] sparse table keys (0 = empty): tables 0 / 1 (ctl->cur), 2 = the copy
    unsigned long long* tcnt;         // [3 x tcap] their counts
    uint64_t cap;
    uint32_t D, tcap, dirs, sort_all;
};

struct DegLocal {                                        // a thread's share of the summary's scalars
    long long dverts = 0, ddegs = 0;
    unsigned long long ck = 0;
    uint32_t mx = 0, dirty = 0;
};

__device__ __forceinline__ uint32_t deg_hash(uint32_t d) { return d * 0x9E3779B1u; }

// slot of `want` lanes in a list: one counter add per wave. Lanes named by the ballot are active.
__device__ __forceinline__ uint32_t wave_slot(bool want, uint32_t* counter) {
    const unsigned long long m = __ballot(want);
    if (!m) return 0;
    const int leader = __ffsll((long long)m) - 1;
    const int lane = (int)__lane_id();
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(m));
    base = __shfl(base, leader, 64);
    return base + (uint32_t)__popcll(m & ((1ull << lane) - 1));
}

// the count word of degree d >= D in table t, inserted when absent (null: the table is full,
// which the host's capacity rule excludes; reported as ctl->overflow). Out of line, like
// dist_global: the path of degrees >= kLdsDeg is cold, and with it inlined into k_deg_close
// ROCm 7.2's clang crashed in its CFG simplification.
__device__ __noinline__ unsigned long long* tab_slot(const DegArgs& g, uint32_t t, uint32_t d, bool insert) {
    uint32_t* keys = g.tkeys + (size_t)t * g.tcap;
    const uint32_t mask = g.tcap - 1;
    uint32_t s = (deg_hash(d) >> 8) & mask;
    for (uint32_t probes = 0; probes < g.tcap; ++probes, s = (s + 1) & mask) {
        uint32_t k = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == 0) {
            if (!insert) return nullptr;
            k = atomicCAS(&keys[s], 0u, d);
            if (k == 0) {
                atomicAdd(&g.ctl->used, 1u);
                k = d;
            }
        }
        if (k == d) return g.tcnt + (size_t)t * g.tcap + s;
    }
    if (insert) atomicOr(&g.ctl->overflow, 1u);
    return nullptr;
}

// count[d] += x (x != 0) in global memory; 0 <-> non-zero transitions move n_degrees (the atomics on
// one word are ordered, and each sees the value it changed)
__device__ __noinline__ void dist_global(const DegArgs& g, uint32_t d, long long x, DegLocal& L) {
    unsigned long long* p = d < g.D ? g.dense + d : tab_slot(g, g.ctl->cur, d, true);
    if (!p) return;
    const unsigned long long old = atomicAdd(p, (unsigned long long)x);
    if (old == 0) ++L.ddegs;
    else if (old + (unsigned long long)x == 0) --L.ddegs;
}

__device__ __forceinline__ void dist_add(const DegArgs& g, int* lds, uint32_t d, int x, DegLocal& L) {
    if (d == 0) return;
    if (d < kLdsDeg) atomicAdd(&lds[d], x);
    else dist_global(g, d, x, L);
}

// v's degree becomes nw (old != nw): everything but the delta list
__device__ __forceinline__ void deg_apply(const DegArgs& g, int* lds, uint32_t v, uint32_t old, uint32_t nw, uint32_t m0,
                                          DegLocal& L) {
    g.degree[v] = nw;
    dist_add(g, lds, old, -1, L);
    dist_add(g, lds, nw, 1, L);
    L.ck += (nw ? pair_mix(v, nw) : 0ull) - (old ? pair_mix(v, old) : 0ull);
    L.dverts += (long long)(nw != 0) - (long long)(old != 0);
    L.mx = max(L.mx, nw);
    if (old == m0 && nw < old) L.dirty = 1;
}

// end of an applying kernel: the workgroup's low degrees, then each wave's scalars
__device__ __forceinline__ void deg_epilogue(const DegArgs& g, int* lds, DegLocal& L) {
    __syncthreads();
    for (uint32_t d = threadIdx.x; d < kLdsDeg; d += kDegThreads) {
        const int x = lds[d];
        if (x) dist_global(g, d, x, L);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        L.dverts += __shfl_down(L.dverts, off, 64);
        L.ddegs += __shfl_down(L.ddegs, off, 64);
        L.ck += __shfl_down(L.ck, off, 64);
        L.mx = max(L.mx, (uint32_t)__shfl_down(L.mx, off, 64));
        L.dirty |= (uint32_t)__shfl_down(L.dirty, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (L.dverts) atomicAdd(&g.ctl->n_vertices, (unsigned long long)L.dverts);
        if (L.ddegs) atomicAdd(&g.ctl->n_degrees, (unsigned long long)L.ddegs);
        if (L.ck) atomicAdd(&g.ctl->checksum, L.ck);
        if (L.mx) atomicMax(&g.ctl->newmax, L.mx);
        if (L.dirty) atomicOr(&g.ctl->dirty, 1u);
    }
}

#define DEG_LDS_INIT(lds)                                                     \
    __shared__ int lds[kLdsDeg];                                              \
    for (uint32_t d_ = threadIdx.x; d_ < kLdsDeg; d_ += kDegThreads) lds[d_] = 0; \
    __syncthreads()

// begin: the window's control words; the sparse table rebuilt without its zero counts when half of
// it is in use. One workgroup.
__global__ __launch_bounds__(kGcThreads) void k_deg_begin(DegArgs g) {
    DegCtl* c = g.ctl;
    __shared__ uint32_t live;
    if (threadIdx.x == 0) {
        c->n_touched = c->n_delta = c->n_risk = c->n_risk_events = c->n_keys = 0;
        c->dirty = c->newmax = c->scanmax = 0;
        c->m0 = c->maxdeg;
        live = 0;
    }
    const uint32_t cur = c->cur, used = c->used;
    if (used * 2ull <= g.tcap) return;                  // (uniform: nothing here writes cur or used before)
    const uint32_t oth = cur ^ 1u;
    uint32_t* ok = g.tkeys + (size_t)oth * g.tcap;
    unsigned long long* oc = g.tcnt + (size_t)oth * g.tcap;
    for (uint32_t s = threadIdx.x; s < g.tcap; s += kGcThreads) {
        atomicExch(&ok[s], 0u);
        atomicExch(&oc[s], 0ull);
    }
    __syncthreads();
    const uint32_t* ck = g.tkeys + (size_t)cur * g.tcap;
    const unsigned long long* cc = g.tcnt + (size_t)cur * g.tcap;
    const uint32_t mask = g.tcap - 1;
    for (uint32_t s = threadIdx.x; s < g.tcap; s += kGcThreads) {
        const uint32_t k = ck[s];
        const unsigned long long n = cc[s];
        if (k == 0 || n == 0) continue;
        atomicAdd(&live, 1u);
        for (uint32_t t = (deg_hash(k) >> 8) & mask;; t = (t + 1) & mask)    // (the keys are distinct; live <= tcap / 2)
            if (atomicCAS(&ok[t], 0u, k) == 0) {
                atomicExch(&oc[t], n);
                break;
            }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        c->cur = oth;
        c->used = live;
    }
}

// count: the window's vertex events into the accumulators
template <typename IdT>
__global__ __launch_bounds__(kDegThreads) void k_deg_count(const IdT* __restrict__ src, const IdT* __restrict__ dst,
                                                           const uint8_t* __restrict__ add, uint32_t n, DegArgs g) {
    __shared__ uint32_t skey[kDegSlots];
    __shared__ unsigned long long sval[kDegSlots];
    bool bad = false;
    const uint32_t tiles = (n + kDegTile - 1) / kDegTile;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {         // (workgroup-uniform)
        for (uint32_t s = threadIdx.x; s < kDegSlots; s += kDegThreads) {
            skey[s] = kInvalid;
            sval[s] = 0;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < kDegEPT; ++k) {
            const uint32_t i = tile * kDegTile + k * kDegThreads + threadIdx.x;
            bool ok = false;
            uint32_t ends[2] = {0, 0};
            unsigned long long val = 1;
            if (i < n) {
                const IdT x = src[i], y = dst[i];
                ok = (uint64_t)x < g.cap && (uint64_t)y < g.cap;                // (a negative int64 is >= 2^63)
                bad |= !ok;
                ends[0] = (uint32_t)x;
                ends[1] = (uint32_t)y;
                if (add && !add[i]) val = 1ull << 32;
            }
#pragma unroll
            for (uint32_t e = 0; e < 2; ++e) {
                const bool on = ok && ((g.dirs >> e) & 1u);                    // bit 0: sources, bit 1: targets
                const uint32_t v = ends[e];
                bool direct = false;
                if (on) {
                    const uint32_t s = deg_hash(v) >> 21;                       // 11 bits: kDegSlots
                    const uint32_t prev = atomicCAS(&skey[s], kInvalid, v);
                    if (prev == kInvalid || prev == v) atomicAdd(&sval[s], val);
                    else direct = true;
                }
                const unsigned long long old = direct ? atomicAdd(&g.acc[v], val) : 1ull;
                const bool first = direct && old == 0;
                const uint32_t at = wave_slot(first, &g.ctl->n_touched);
                if (first) g.touched[at] = v;
            }
        }
        __syncthreads();
        for (uint32_t s = threadIdx.x; s < kDegSlots; s += kDegThreads) {       // (uniform trip count)
            const uint32_t v = skey[s];
            const bool has = v != kInvalid;
            const unsigned long long old = has ? atomicAdd(&g.acc[v], sval[s]) : 1ull;
            const bool first = has && old == 0;
            const uint32_t at = wave_slot(first, &g.ctl->n_touched);
            if (first) g.touched[at] = v;
        }
        __syncthreads();
    }
    if (bad) atomicOr(&g.ctl->range, 1u);
}

// close: the touched list
__global__ __launch_bounds__(kDegThreads) void k_deg_close(DegArgs g) {
    DEG_LDS_INIT(lds);
    DegLocal L;
    const uint32_t nt = g.ctl->n_touched, m0 = g.ctl->m0;
    const bool failed = g.ctl->range != 0;
    uint32_t n_risk = 0, n_events = 0;
    for (uint32_t base = blockIdx.x * blockDim.x; base < nt; base += gridDim.x * blockDim.x) {   // (wave-uniform)
        const uint32_t i = base + threadIdx.x;
        bool changed = false;
        uint32_t v = 0, nw = 0, old = 0;
        unsigned long long a = 0;
        if (i < nt) {
            v = g.touched[i];
            a = g.acc[v];
            g.acc[v] = 0;
            old = g.degree[v];
        }
        const uint32_t plus = (uint32_t)a, minus = (uint32_t)(a >> 32);
        const bool live = i < nt && !failed;
        const bool risk = live && minus > old;           // else no prefix of the window's events can clamp
        if (live && !risk) {
            nw = old + plus - minus;
            changed = nw != old;
        }
        if (changed) deg_apply(g, lds, v, old, nw, m0, L);
        if (risk) {
            atomicOr(&g.bits[v >> 5], 1u << (v & 31));
            n_risk += 1;
            n_events += plus + minus;
        }
        const uint32_t at = wave_slot(changed, &g.ctl->n_delta);
        if (changed) {
            g.dv[at] = v;
            g.dd[at] = nw;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n_risk += __shfl_down(n_risk, off, 64);
        n_events += __shfl_down(n_events, off, 64);
    }
    if ((threadIdx.x & 63) == 0 && n_risk) {
        atomicAdd(&g.ctl->n_risk, n_risk);
        atomicAdd(&g.ctl->n_risk_events, n_events);
    }
    deg_epilogue(g, lds, L);
}

// exact path, keys: vertex << shift | position << 1 | sign (1 = addition); position = 2 x event + end
template <typename IdT, bool ALL>
__global__ __launch_bounds__(kDegThreads) void k_deg_keys(const IdT* __restrict__ src, const IdT* __restrict__ dst,
                                                          const uint8_t* __restrict__ add, uint32_t n, uint32_t shift,
                                                          uint64_t* __restrict__ keys, uint32_t key_cap, DegArgs g) {
    bool bad = false;
    const uint32_t both = g.dirs == 3u;
    for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {     // (wave-uniform)
        const uint32_t i = base + threadIdx.x;
        bool ok = false;
        uint32_t ends[2] = {0, 0};
        uint64_t sign = 1;
        if (i < n) {
            const IdT x = src[i], y = dst[i];
            ok = (uint64_t)x < g.cap && (uint64_t)y < g.cap;
            bad |= !ok;
            ends[0] = (uint32_t)x;
            ends[1] = (uint32_t)y;
            if (add && !add[i]) sign = 0;
        }
#pragma unroll
        for (uint32_t e = 0; e < 2; ++e) {
            if (!((g.dirs >> e) & 1u)) continue;         // (uniform)
            const uint32_t v = ends[e];
            const uint64_t key = ((uint64_t)v << shift) | ((uint64_t)(2 * (uint64_t)i + e) << 1) | sign;
            if (ALL) {                                   // a fixed place per vertex event; a bad event's key is never applied
                if (i < n) keys[both ? 2 * (size_t)i + e : i] = ok ? key : 0;
            } else {
                const bool want = ok && ((g.bits[v >> 5] >> (v & 31)) & 1u);
                const uint32_t at = wave_slot(want, &g.ctl->n_keys);
                if (want && at < key_cap) keys[at] = key;
            }
        }
    }
    if (ALL && bad) atomicOr(&g.ctl->range, 1u);
}

__global__ __launch_bounds__(kDegThreads) void k_deg_elems(const uint64_t* __restrict__ keys, uint32_t n, uint32_t shift,
                                                           DegEl* __restrict__ el) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint64_t k = keys[i];
        DegEl e;
        e.a = (k & 1) ? 1 : -1;
        e.b = 0;
        e.head = (i == 0 || (keys[i - 1] >> shift) != (k >> shift)) ? 1u : 0u;
        e.pad = 0;
        el[i] = e;
    }
}

// exact path, apply: the last element of a vertex's run holds its (A, B)
__global__ __launch_bounds__(kDegThreads) void k_deg_exact(const uint64_t* __restrict__ keys, const DegEl* __restrict__ sc,
                                                           uint32_t n, uint32_t shift, DegArgs g) {
    DEG_LDS_INIT(lds);
    DegLocal L;
    const uint32_t m0 = g.ctl->m0;
    const bool failed = g.ctl->range != 0;
    for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {     // (wave-uniform)
        const uint32_t i = base + threadIdx.x;
        bool changed = false;
        uint32_t v = 0, nw = 0;
        if (i < n && !failed) {
            const uint64_t k = keys[i];
            v = (uint32_t)(k >> shift);
            if (v < g.cap && (i + 1 == n || (uint32_t)(keys[i + 1] >> shift) != v)) {
                const DegEl e = sc[i];
                const uint32_t old = g.degree[v];
                const long long x = max((long long)old + e.a, (long long)e.b);
                nw = (uint32_t)x;
                changed = nw != old;
                if (changed) deg_apply(g, lds, v, old, nw, m0, L);
                if (!g.sort_all) atomicAnd(&g.bits[v >> 5], ~(1u << (v & 31)));
            }
        }
        const uint32_t at = wave_slot(changed, &g.ctl->n_delta);
        if (changed) {
            g.dv[at] = v;
            g.dd[at] = nw;
        }
    }
    deg_epilogue(g, lds, L);
}

// the largest degree with a count, when a vertex that held the maximum lost degree
__global__ __launch_bounds__(kDegThreads) void k_deg_maxscan(DegArgs g) {
    if (!g.ctl->dirty) return;
    const uint32_t cur = g.ctl->cur;
    uint32_t mx = 0;
    const uint32_t total = g.D + g.tcap;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        if (i < g.D) {
            if (g.dense[i]) mx = max(mx, i);
        } else {
            const size_t s = (size_t)cur * g.tcap + (i - g.D);
            if (g.tkeys[s] && g.tcnt[s]) mx = max(mx, g.tkeys[s]);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = max(mx, (uint32_t)__shfl_down(mx, off, 64));
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(&g.ctl->scanmax, mx);
}

__global__ void k_deg_finish(DegArgs g, unsigned long long* __restrict__ out) {
    DegCtl* c = g.ctl;
    const uint32_t mx = c->dirty ? c->scanmax : max(c->m0, c->newmax);
    c->maxdeg = mx;
    if (out) {
        out[0] = c->n_vertices;
        out[1] = c->n_degrees;
        out[2] = mx;
        out[3] = c->checksum;
    }
}

// the distribution as it is now, copied for the next distribution delta
__global__ __launch_bounds__(kDegThreads) void k_deg_snapshot(DegArgs g) {
    const uint32_t cur = g.ctl->cur;
    const uint32_t total = g.D + g.tcap;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        if (i < g.D) {
            g.sdense[i] = g.dense[i];
        } else {
            const uint32_t s = i - g.D;
            g.tkeys[2 * (size_t)g.tcap + s] = g.tkeys[(size_t)cur * g.tcap + s];
            g.tcnt[2 * (size_t)g.tcap + s] = g.tcnt[(size_t)cur * g.tcap + s];
        }
    }
}

// distribution emission, unordered: delta = 0: keys with a count; 1: keys whose count differs from the copy's
__global__ __launch_bounds__(kDegThreads) void k_deg_dist(DegArgs g, int delta, uint32_t* __restrict__ od,
                                                          unsigned long long* __restrict__ oc) {
    const uint32_t cur = g.ctl->cur;
    const uint32_t total = g.D + 2 * g.tcap;
    for (uint32_t base = blockIdx.x * blockDim.x; base < total; base += gridDim.x * blockDim.x) {  // (wave-uniform)
        const uint32_t i = base + threadIdx.x;
        bool want = false;
        uint32_t d = 0;
        unsigned long long c = 0;
        if (i < g.D) {
            d = i;
            c = g.dense[i];
            want = delta ? c != g.sdense[i] : c != 0;
        } else if (i < g.D + g.tcap) {
            const size_t s = (size_t)cur * g.tcap + (i - g.D);
            d = g.tkeys[s];
            if (d) {
                c = g.tcnt[s];
                if (delta) {
                    const unsigned long long* p = tab_slot(g, 2, d, false);
                    want = c != (p ? *p : 0ull);
                } else {
                    want = c != 0;
                }
            }
        } else if (i < total && delta) {                 // a key of the copy the table no longer holds: its count is 0
            const size_t s = 2 * (size_t)g.tcap + (i - g.D - g.tcap);
            d = g.tkeys[s];
            want = d && g.tcnt[s] && !tab_slot(g, cur, d, false);
        }
        const uint32_t at = wave_slot(want, &g.ctl->n_emit);
        if (want) {
            od[at] = d;
            oc[at] = c;
        }
    }
}

// the whole degree map, unordered
__global__ __launch_bounds__(kDegThreads) void k_deg_map(DegArgs g, uint32_t* __restrict__ ov, uint32_t* __restrict__ od) {
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < g.cap; base += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t v = base + threadIdx.x;
        const uint32_t d = v < g.cap ? g.degree[v] : 0;
        const uint32_t at = wave_slot(d != 0, &g.ctl->n_emit);
        if (d) {
            ov[at] = (uint32_t)v;
            od[at] = d;
        }
    }
}

template <typename IdT>
__global__ __launch_bounds__(kDegThreads) void k_deg_widen(const uint32_t* __restrict__ in, IdT* __restrict__ out, uint32_t n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = (IdT)in[i];
}

template <typename IdT>
__global__ __launch_bounds__(kDegThreads) void k_deg_find(const IdT* __restrict__ ids, uint32_t* __restrict__ out, uint64_t n,
                                                          DegArgs g) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t v = (uint64_t)ids[i];
        out[i] = v < g.cap ? g.degree[v] : 0;
    }
}

// restore, step 1: the snapshot is checked without touching the summary (the at-risk bitmap, zero
// between windows, finds repeated vertices; step 3 zeroes it again)
template <typename IdT>
__global__ __launch_bounds__(kDegThreads) void k_deg_restore_check(const IdT* __restrict__ vs, const uint32_t* __restrict__ ds,
                                                                   uint32_t n, DegArgs g) {
    unsigned long long sum = 0;
    uint32_t mx = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint64_t v = (uint64_t)vs[i];
        const uint32_t d = ds[i];
        if (v >= g.cap) {
            atomicOr(&g.ctl->range, 1u);
            continue;
        }
        if (d == 0) atomicOr(&g.ctl->bad_zero, 1u);
        const uint32_t bit = 1u << (v & 31);
        if (atomicOr(&g.bits[v >> 5], bit) & bit) atomicOr(&g.ctl->bad_dup, 1u);
        sum += d;
        mx = max(mx, d);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_down(sum, off, 64);
        mx = max(mx, (uint32_t)__shfl_down(mx, off, 64));
    }
    if ((threadIdx.x & 63) == 0 && mx) {
        atomicAdd(&g.ctl->vsum, sum);
        atomicMax(&g.ctl->vmax, mx);
    }
}

template <typename IdT>
__global__ __launch_bounds__(kDegThreads) void k_deg_restore_bits(const IdT* __restrict__ vs, uint32_t n, DegArgs g) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint64_t v = (uint64_t)vs[i];
        if (v < g.cap) g.bits[v >> 5] = 0;
    }
}

template <typename IdT>
__global__ __launch_bounds__(kDegThreads) void k_deg_restore_apply(const IdT* __restrict__ vs, const uint32_t* __restrict__ ds,
                                                                   uint32_t n, DegArgs g) {
    DEG_LDS_INIT(lds);
    DegLocal L;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        deg_apply(g, lds, (uint32_t)vs[i], 0, ds[i], 0xFFFFFFFFu, L);
    deg_epilogue(g, lds, L);
}

}  // namespace gsgpu

using namespace gsgpu;

struct gs_deg {
    uint64_t cap = 0;
    uint32_t id_bits = 64, vbits = 1, flags = 0, dirs = 3, D = 0, tcap = 0;
    bool sort_all = false;
    int device = 0;
    Stream own;
    hipStream_t stream = nullptr;
    DevBuf<uint32_t> degree, touched, bits, dlist, tkeys;
    DevBuf<unsigned long long> acc, dense, tcnt, wstats;
    DevBuf<DegCtl> ctl;
    Pinned<> hbuf;                             // pinned mirror: control words, then the call's window statistics
    size_t hbuf_bytes = 0;
    DevBuf<> tmp;                              // exact path: keys x 2, elements x 2, sort / scan temporaries
    DevBuf<> stage;                            // host inputs of one window
    DevBuf<> ebuf;                             // emissions
    // host-side bounds (never read from the device inside a fold)
    uint64_t restored_max = 0;                 // largest degree of the last restore
    uint64_t events = 0;                       // vertex-event bound: events folded since reset / restore
    long double sum_bound = 0;                 // restored degree sum + 2 x events
    uint64_t path[4] = {0, 0, 0, 0};           // windows, windows that took the exact path, vertex events, those sorted
};

namespace {

constexpr uint64_t kDegMaxCap = 0xFFFFFFFFull;
constexpr uint64_t kDegMaxWindow = (1ull << 30) - 1;  // 2 x events fit an int (hipcub) and DegEl's int32

int dcheck(gs_deg_t* h, const char* fn) { return h ? GS_OK : fail(GS_ERR_INVALID, "%s: null handle", fn); }

unsigned dgrid(uint64_t items) {
    const uint64_t b = (items + kDegThreads - 1) / kDegThreads;
    return (unsigned)std::min<uint64_t>(std::max<uint64_t>(b, 1), kDegMaxBlocks);
}

size_t dup256(size_t x) { return (x + 255) & ~(size_t)255; }

DegArgs dargs(gs_deg_t* h) {
    DegArgs g;
    g.ctl = h->ctl.get();
    g.degree = h->degree.get();
    g.acc = h->acc.get();
    g.touched = h->touched.get();
    g.bits = h->bits.get();
    g.dv = h->dlist.get();
    g.dd = h->dlist.get() + h->cap;
    g.dense = h->dense.get();
    g.sdense = h->dense.get() + h->D;
    g.tkeys = h->tkeys.get();
    g.tcnt = h->tcnt.get();
    g.cap = h->cap;
    g.D = h->D;
    g.tcap = h->tcap;
    g.dirs = h->dirs;
    g.sort_all = h->sort_all ? 1u : 0u;
    return g;
}

size_t bit_words(uint64_t cap) { return (size_t)((cap + 31) / 32); }

// an empty summary (enqueued)
int dclear(gs_deg_t* h) {
    GS_HIP(hipMemsetAsync(h->degree.get(), 0, (size_t)h->cap * 4, h->stream));
    if (!h->sort_all) GS_HIP(hipMemsetAsync(h->acc.get(), 0, (size_t)h->cap * 8, h->stream));
    GS_HIP(hipMemsetAsync(h->bits.get(), 0, bit_words(h->cap) * 4, h->stream));
    GS_HIP(hipMemsetAsync(h->dense.get(), 0, (size_t)h->D * 2 * 8, h->stream));
    GS_HIP(hipMemsetAsync(h->tkeys.get(), 0, (size_t)h->tcap * 3 * 4, h->stream));
    GS_HIP(hipMemsetAsync(h->tcnt.get(), 0, (size_t)h->tcap * 3 * 8, h->stream));
    GS_HIP(hipMemsetAsync(h->ctl.get(), 0, sizeof(DegCtl), h->stream));
    h->restored_max = 0;
    h->events = 0;
    h->sum_bound = 0;
    return GS_OK;
}

int dpinned(gs_deg_t* h, size_t bytes) {
    if (h->hbuf_bytes >= bytes) return GS_OK;
    GS_TRY(h->hbuf.alloc(bytes, "degree results"));
    h->hbuf_bytes = bytes;
    return GS_OK;
}

// the control words on the host (a host wait)
int dread(gs_deg_t* h, DegCtl& c) {
    GS_TRY(dpinned(h, sizeof(DegCtl)));
    GS_HIP(hipMemcpyAsync(h->hbuf.get(), h->ctl.get(), sizeof(DegCtl), hipMemcpyDeviceToHost, h->stream));
    GS_HIP(hipStreamSynchronize(h->stream));
    memcpy(&c, h->hbuf.get(), sizeof(DegCtl));
    return GS_OK;
}

// Limits checked on the host before a window of n events is folded: degrees are 32 bits wide, and
// the sparse table holds at most tcap / 4 distinct degrees >= D at a time (k distinct degrees need a
// degree sum of at least k^2 / 2 and of at least k x D; there are at most `cap` vertices).
int dlimits(gs_deg_t* h, uint64_t n, const char* fn) {
    const uint64_t ev = h->events + n;
    if ((long double)h->restored_max + 2.0L * (long double)ev > 4294967295.0L)
        return fail(GS_ERR_CAPACITY, "%s: a degree could pass 2^32 - 1 (restored maximum %llu + 2 x %llu events)", fn,
                    (unsigned long long)h->restored_max, (unsigned long long)ev);
    const long double s = h->sum_bound + 2.0L * (long double)n;
    long double k = std::min<long double>((long double)h->cap, s / (long double)h->D);
    k = std::min<long double>(k, std::sqrt((double)(2.0L * s)) + 1.0L);
    if (k > (long double)(h->tcap / 4))
        return fail(GS_ERR_CAPACITY, "%s: more than %u distinct degrees >= %u are possible", fn, h->tcap / 4, h->D);
    return GS_OK;
}

struct DegScratch {
    uint64_t *ka = nullptr, *kb = nullptr;
    DegEl *ea = nullptr, *eb = nullptr;
    void* tmp = nullptr;
    size_t tmp_bytes = 0, sort_bytes = 0, scan_bytes = 0;
    uint32_t cap = 0;
};

// scratch of the exact path for up to n keys
int dscratch(gs_deg_t* h, uint64_t n, uint32_t end_bit, DegScratch& s) {
    n = std::max<uint64_t>(n, 1);
    GS_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, s.sort_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)n, 0,
                                              (int)end_bit, h->stream));
    GS_HIP(hipcub::DeviceScan::InclusiveScan(nullptr, s.scan_bytes, (const DegEl*)nullptr, (DegEl*)nullptr, DegOp(), (int)n,
                                              h->stream));
    s.tmp_bytes = std::max(s.sort_bytes, s.scan_bytes);
    const size_t kbytes = dup256(n * 8), ebytes = dup256(n * sizeof(DegEl));
    GS_TRY(h->tmp.grow(2 * kbytes + 2 * ebytes + dup256(s.tmp_bytes), "degree exact-path scratch", h->stream));
    char* p = static_cast<char*>(h->tmp.get());
    s.ka = reinterpret_cast<uint64_t*>(p);
    s.kb = reinterpret_cast<uint64_t*>(p + kbytes);
    s.ea = reinterpret_cast<DegEl*>(p + 2 * kbytes);
    s.eb = reinterpret_cast<DegEl*>(p + 2 * kbytes + ebytes);
    s.tmp = p + 2 * kbytes + 2 * ebytes;
    s.cap = (uint32_t)n;
    return GS_OK;
}

uint32_t bits_for(uint64_t x) {                 // bits that hold every value below x
    uint32_t b = 1;
    while (b < 64 && (1ull << b) < x) ++b;
    return b;
}

// one window of n device events (enqueued; a window with deletions whose close finds at-risk
// vertices waits once for their event count)
int dwindow(gs_deg_t* h, const void* src, const void* dst, const uint8_t* add, uint32_t n, bool snapshot,
            unsigned long long* stats_out) {
    const DegArgs g = dargs(h);
    const dim3 block(kDegThreads);
    hipLaunchKernelGGL(k_deg_begin, dim3(1), dim3(kGcThreads), 0, h->stream, g);
    if (snapshot) hipLaunchKernelGGL(k_deg_snapshot, dim3(dgrid((uint64_t)h->D + h->tcap)), block, 0, h->stream, g);
    GS_HIP(hipGetLastError());
    const uint32_t ndirs = h->dirs == 3 ? 2 : 1;
    const uint32_t shift = bits_for(2ull * std::max<uint32_t>(n, 1)) + 1;
    const uint32_t end_bit = h->vbits + shift;
    uint32_t nkeys = 0;
    bool all = false;
    if (n && h->sort_all) {
        nkeys = n * ndirs;
        all = true;
    } else if (n) {
        const uint32_t tiles = (n + kDegTile - 1) / kDegTile;
        const dim3 grid(std::min<uint32_t>(tiles, kDegMaxBlocks));
        if (h->id_bits == 32)
            hipLaunchKernelGGL(k_deg_count<uint32_t>, grid, block, 0, h->stream, (const uint32_t*)src, (const uint32_t*)dst, add, n, g);
        else
            hipLaunchKernelGGL(k_deg_count<int64_t>, grid, block, 0, h->stream, (const int64_t*)src, (const int64_t*)dst, add, n, g);
        hipLaunchKernelGGL(k_deg_close, dim3(dgrid(std::min<uint64_t>(h->cap, (uint64_t)n * ndirs))), block, 0, h->stream, g);
        GS_HIP(hipGetLastError());
        if (add) {                               // only deletions can put a vertex at risk
            DegCtl c;
            GS_TRY(dread(h, c));
            nkeys = c.n_risk_events;
        }
    }
    h->path[0] += 1;
    h->path[2] += (uint64_t)n * ndirs;
    if (nkeys) {
        h->path[1] += 1;
        h->path[3] += nkeys;
        DegScratch s;
        GS_TRY(dscratch(h, nkeys, end_bit, s));
        const dim3 egrid(dgrid(n)), kgrid(dgrid(nkeys));
#define DEG_KEYS(IdT, ALLV)                                                                                         \
        hipLaunchKernelGGL((k_deg_keys<IdT, ALLV>), egrid, block, 0, h->stream, (const IdT*)src, (const IdT*)dst, add, n, \
                           shift, s.ka, s.cap, g)
        if (h->id_bits == 32) { if (all) DEG_KEYS(uint32_t, true); else DEG_KEYS(uint32_t, false); }
        else { if (all) DEG_KEYS(int64_t, true); else DEG_KEYS(int64_t, false); }
#undef DEG_KEYS
        GS_HIP(hipGetLastError());
        size_t bytes = s.tmp_bytes;
        GS_HIP(hipcub::DeviceRadixSort::SortKeys(s.tmp, bytes, (const uint64_t*)s.ka, s.kb, (int)nkeys, 0, (int)end_bit, h->stream));
        hipLaunchKernelGGL(k_deg_elems, kgrid, block, 0, h->stream, (const uint64_t*)s.kb, nkeys, shift, s.ea);
        GS_HIP(hipGetLastError());
        // An inclusive scan's output i is x0 (+) ... (+) xi in index order by definition; hipcub's
        // DeviceScan asks only that the operator be associative (DegOp is; it is not commutative),
        // so element i is the ordered composition of its vertex's run up to i.
        bytes = s.tmp_bytes;
        GS_HIP(hipcub::DeviceScan::InclusiveScan(s.tmp, bytes, (const DegEl*)s.ea, s.eb, DegOp(), (int)nkeys, h->stream));
        hipLaunchKernelGGL(k_deg_exact, kgrid, block, 0, h->stream, (const uint64_t*)s.kb, (const DegEl*)s.eb, nkeys, shift, g);
        GS_HIP(hipGetLastError());
    }
    if (add) hipLaunchKernelGGL(k_deg_maxscan, dim3(dgrid((uint64_t)h->D + h->tcap)), block, 0, h->stream, g);
    hipLaunchKernelGGL(k_deg_finish, dim3(1), dim3(1), 0, h->stream, g, stats_out);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

// the window's events where the kernels can read them
int dinput(gs_deg_t* h, const void* src, const void* dst, const uint8_t* add, uint64_t off, uint64_t n, uint64_t wmax, bool dev,
           const void*& a, const void*& b, const uint8_t*& c) {
    const size_t esz = h->id_bits / 8;
    if (n == 0) {
        a = b = nullptr;
        c = nullptr;
        return GS_OK;
    }
    if (dev) {
        a = static_cast<const char*>(src) + off * esz;
        b = static_cast<const char*>(dst) + off * esz;
        c = add ? add + off : nullptr;
        return GS_OK;
    }
    char* s0 = static_cast<char*>(h->stage.get());
    char* s1 = s0 + dup256(wmax * esz);
    char* s2 = s1 + dup256(wmax * esz);
    GS_HIP(hipMemcpyAsync(s0, static_cast<const char*>(src) + off * esz, n * esz, hipMemcpyDefault, h->stream));
    GS_HIP(hipMemcpyAsync(s1, static_cast<const char*>(dst) + off * esz, n * esz, hipMemcpyDefault, h->stream));
    if (add) GS_HIP(hipMemcpyAsync(s2, add + off, n, hipMemcpyDefault, h->stream));
    a = s0;
    b = s1;
    c = add ? reinterpret_cast<const uint8_t*>(s2) : nullptr;
    return GS_OK;
}

int dfold(gs_deg_t* h, const char* fn, const void* src, const void* dst, const uint8_t* add, uint64_t n, uint64_t window_edges,
          gs_deg_window_stats* stats, uint64_t nw) {
    const uint64_t wmax = std::min(n, window_edges);
    if (wmax > kDegMaxWindow) return fail(GS_ERR_UNSUPPORTED, "%s: windows of more than 2^30 - 1 events", fn);
    if (h->vbits + bits_for(2 * std::max<uint64_t>(wmax, 1)) + 1 > 64)
        return fail(GS_ERR_UNSUPPORTED, "%s: vertex, position and sign do not fit a 64-bit key", fn);
    GS_TRY(dlimits(h, n, fn));
    DeviceGuard g(h->device);
    const bool dev = is_device_pointer(src) && is_device_pointer(dst) && (!add || is_device_pointer(add));
    if (!dev && wmax) GS_TRY(h->stage.grow(2 * dup256(wmax * (h->id_bits / 8)) + dup256(wmax), "degree input staging", h->stream));
    GS_TRY(h->wstats.grow(std::max<uint64_t>(nw, 1) * 4, "degree window statistics", h->stream));
    if (h->sort_all) {                           // the scratch of the largest window, before anything is enqueued
        DegScratch s;
        GS_TRY(dscratch(h, wmax * (h->dirs == 3 ? 2 : 1), 64, s));
    }
    GS_HIP(hipMemsetAsync(&h->ctl.get()->range, 0, 2 * sizeof(uint32_t), h->stream));   // range, overflow
    for (uint64_t w = 0; w < nw; ++w) {
        const uint64_t off = w * window_edges, m = std::min(window_edges, n - off);
        const void *a, *b;
        const uint8_t* c;
        GS_TRY(dinput(h, src, dst, add, off, m, wmax, dev, a, b, c));
        GS_TRY(dwindow(h, a, b, c, (uint32_t)m, w + 1 == nw, h->wstats.get() + 4 * w));
    }
    h->events += n;
    h->sum_bound += 2.0L * (long double)n;
    GS_TRY(dpinned(h, sizeof(DegCtl) + nw * 32));
    char* hb = static_cast<char*>(h->hbuf.get());
    GS_HIP(hipMemcpyAsync(hb, h->ctl.get(), sizeof(DegCtl), hipMemcpyDeviceToHost, h->stream));
    if (nw) GS_HIP(hipMemcpyAsync(hb + sizeof(DegCtl), h->wstats.get(), nw * 32, hipMemcpyDeviceToHost, h->stream));
    GS_HIP(hipStreamSynchronize(h->stream));
    DegCtl c;
    memcpy(&c, hb, sizeof(DegCtl));
    if (c.range) return fail(GS_ERR_RANGE, "%s: a vertex id outside [0, %llu); its window and the later ones are not folded",
                             fn, (unsigned long long)h->cap);
    if (c.overflow) return fail(GS_ERR_CAPACITY, "%s: the sparse degree table overflowed", fn);
    if (stats) memcpy(stats, hb + sizeof(DegCtl), nw * 32);
    return GS_OK;
}

// an unordered (key, value) emission of n pairs in ebuf -> ordered by key, written to the caller's
// arrays (host or device); keys id_bits wide when wide_keys, else uint32
int dsorted_out(gs_deg_t* h, uint32_t* k, uint32_t* v, uint32_t n, uint32_t key_bits, void* okeys, void* ovals) {
    if (!n) return GS_OK;
    DevBuf<> scratch;
    size_t sort_bytes = 0;
    GS_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                               (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, 0, (int)key_bits, h->stream));
    const size_t a4 = dup256((size_t)n * 4), a8 = dup256((size_t)n * 8);
    GS_TRY(scratch.grow(2 * a4 + a8 + dup256(sort_bytes), "degree emission scratch"));
    char* p = static_cast<char*>(scratch.get());
    uint32_t* sk = reinterpret_cast<uint32_t*>(p);
    uint32_t* sv = reinterpret_cast<uint32_t*>(p + a4);
    int64_t* wide = reinterpret_cast<int64_t*>(p + 2 * a4);
    GS_HIP(hipcub::DeviceRadixSort::SortPairs(p + 2 * a4 + a8, sort_bytes, (const uint32_t*)k, sk, (const uint32_t*)v, sv, (int)n,
                                               0, (int)key_bits, h->stream));
    if (h->id_bits == 64) {
        hipLaunchKernelGGL(k_deg_widen<int64_t>, dim3(dgrid(n)), dim3(kDegThreads), 0, h->stream, (const uint32_t*)sk, wide, n);
        GS_HIP(hipGetLastError());
        GS_HIP(hipMemcpyAsync(okeys, wide, (size_t)n * 8, hipMemcpyDefault, h->stream));
    } else {
        GS_HIP(hipMemcpyAsync(okeys, sk, (size_t)n * 4, hipMemcpyDefault, h->stream));
    }
    GS_HIP(hipMemcpyAsync(ovals, sv, (size_t)n * 4, hipMemcpyDefault, h->stream));
    GS_HIP(hipStreamSynchronize(h->stream));     // (scratch is freed on return)
    return GS_OK;
}

int demit_degrees(gs_deg_t* h, const char* fn, bool delta, void* vertices, uint32_t* degrees, uint64_t cap, uint64_t* n_out) {
    GS_TRY(dcheck(h, fn));
    if (!n_out) return fail(GS_ERR_INVALID, "%s: null n_out", fn);
    DeviceGuard dg(h->device);
    const DegArgs g = dargs(h);
    uint32_t *k, *v;
    DegCtl c;
    if (delta) {
        GS_TRY(dread(h, c));
        k = g.dv;
        v = g.dd;
        *n_out = c.n_delta;
    } else {
        GS_TRY(h->ebuf.grow((size_t)h->cap * 8, "degree emission", h->stream));
        k = static_cast<uint32_t*>(h->ebuf.get());
        v = k + h->cap;
        GS_HIP(hipMemsetAsync(&h->ctl.get()->n_emit, 0, 4, h->stream));
        hipLaunchKernelGGL(k_deg_map, dim3(dgrid(h->cap)), dim3(kDegThreads), 0, h->stream, g, k, v);
        GS_HIP(hipGetLastError());
        GS_TRY(dread(h, c));
        *n_out = c.n_emit;
    }
    if (cap < *n_out) return fail(GS_ERR_CAPACITY, "%s: %llu entries, capacity %llu", fn, (unsigned long long)*n_out,
                                  (unsigned long long)cap);
    if (*n_out && (!vertices || !degrees)) return fail(GS_ERR_INVALID, "%s: null output", fn);
    return dsorted_out(h, k, v, (uint32_t)*n_out, h->vbits, vertices, degrees);
}

int demit_dist(gs_deg_t* h, const char* fn, int delta, uint32_t* degrees, uint64_t* counts, uint64_t cap, uint64_t* n_out) {
    GS_TRY(dcheck(h, fn));
    if (!n_out) return fail(GS_ERR_INVALID, "%s: null n_out", fn);
    DeviceGuard dg(h->device);
    const DegArgs g = dargs(h);
    const size_t slots = (size_t)h->D + 2 * (size_t)h->tcap;
    GS_TRY(h->ebuf.grow(std::max<size_t>((size_t)h->cap * 8, slots * 12 + 256), "degree emission", h->stream));
    unsigned long long* oc = static_cast<unsigned long long*>(h->ebuf.get());
    uint32_t* od = reinterpret_cast<uint32_t*>(oc + slots);
    GS_HIP(hipMemsetAsync(&h->ctl.get()->n_emit, 0, 4, h->stream));
    hipLaunchKernelGGL(k_deg_dist, dim3(dgrid(slots)), dim3(kDegThreads), 0, h->stream, g, delta, od, oc);
    GS_HIP(hipGetLastError());
    DegCtl c;
    GS_TRY(dread(h, c));
    const uint64_t n = c.n_emit;
    *n_out = n;
    if (cap < n) return fail(GS_ERR_CAPACITY, "%s: %llu keys, capacity %llu", fn, (unsigned long long)n, (unsigned long long)cap);
    if (!n) return GS_OK;
    if (!degrees || !counts) return fail(GS_ERR_INVALID, "%s: null output", fn);
    // a distribution has few keys (k distinct degrees need k^2 / 2 vertex events): ordered on the host
    std::vector<uint32_t> hd(n);
    std::vector<unsigned long long> hc(n);
    GS_HIP(hipMemcpyAsync(hd.data(), od, n * 4, hipMemcpyDeviceToHost, h->stream));
    GS_HIP(hipMemcpyAsync(hc.data(), oc, n * 8, hipMemcpyDeviceToHost, h->stream));
    GS_HIP(hipStreamSynchronize(h->stream));
    std::vector<uint32_t> order(n);
    for (uint64_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return hd[x] < hd[y]; });
    std::vector<uint32_t> sd(n);
    std::vector<uint64_t> sc(n);
    for (uint64_t i = 0; i < n; ++i) {
        sd[i] = hd[order[i]];
        sc[i] = hc[order[i]];
    }
    GS_HIP(hipMemcpy(degrees, sd.data(), n * 4, hipMemcpyDefault));
    GS_HIP(hipMemcpy(counts, sc.data(), n * 8, hipMemcpyDefault));
    return GS_OK;
}

}  // namespace

extern "C" {

int gs_deg_create(gs_deg_t** out, uint64_t vertex_capacity, uint32_t id_bits, int device, uint32_t flags, uint32_t dense_degrees) {
    if (!out) return fail(GS_ERR_INVALID, "gs_deg_create: null out");
    *out = nullptr;
    if (flags & ~(uint32_t)(GS_DEG_OUT | GS_DEG_IN | GS_DEG_SORT_ALL | GS_DEG_COUNT)) return fail(GS_ERR_INVALID, "gs_deg_create: unknown flags 0x%x", flags);
    if ((flags & GS_DEG_SORT_ALL) && (flags & GS_DEG_COUNT)) return fail(GS_ERR_INVALID, "gs_deg_create: GS_DEG_SORT_ALL and GS_DEG_COUNT exclude each other");
    if (id_bits != 32 && id_bits != 64) return fail(GS_ERR_INVALID, "gs_deg_create: id_bits must be 32 or 64");
    if (vertex_capacity == 0 || vertex_capacity > kDegMaxCap)
        return fail(GS_ERR_INVALID, "gs_deg_create: vertex_capacity must be in [1, 2^32 - 1]");
    if (dense_degrees > (1u << 28)) return fail(GS_ERR_INVALID, "gs_deg_create: dense_degrees above 2^28");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return fail(GS_ERR_HIP, "gs_deg_create: no HIP device available");
    }
    if (device < 0 || device >= ndev) return fail(GS_ERR_INVALID, "gs_deg_create: device %d of %d", device, ndev);
    DeviceGuard g(device);
    gs_deg_t* h = new gs_deg_t();
    struct Destroy { void operator()(gs_deg_t* p) const { (void)gs_deg_destroy(p); } };
    std::unique_ptr<gs_deg_t, Destroy> guard(h);
    h->cap = vertex_capacity;
    h->id_bits = id_bits;
    h->flags = flags;
    h->dirs = flags & (GS_DEG_OUT | GS_DEG_IN);
    if (h->dirs == 0) h->dirs = 3;
    h->sort_all = (flags & GS_DEG_COUNT) == 0;          // the default by measurement: sort everything
    h->device = device;
    h->D = std::max<uint32_t>(dense_degrees ? dense_degrees : kDegDefaultDense, 2);
    h->vbits = bits_for(vertex_capacity);
    if (h->vbits > 32) h->vbits = 32;
    h->tcap = 256;
    while (h->tcap < kDegMaxTable && h->tcap < 4 * vertex_capacity) h->tcap <<= 1;
    GS_TRY(h->own.create());
    h->stream = h->own;
    const size_t cap = (size_t)vertex_capacity;
    GS_TRY(h->degree.grow(cap, "gs_deg_create: degrees"));
    GS_TRY(h->acc.grow(h->sort_all ? 1 : cap, "gs_deg_create: window accumulators"));
    GS_TRY(h->touched.grow(h->sort_all ? 1 : cap, "gs_deg_create: touched list"));
    GS_TRY(h->bits.grow(bit_words(vertex_capacity), "gs_deg_create: at-risk bitmap"));
    GS_TRY(h->dlist.grow(2 * cap, "gs_deg_create: degree delta"));
    GS_TRY(h->dense.grow((size_t)h->D * 2, "gs_deg_create: dense counts"));
    GS_TRY(h->tkeys.grow((size_t)h->tcap * 3, "gs_deg_create: sparse table keys"));
    GS_TRY(h->tcnt.grow((size_t)h->tcap * 3, "gs_deg_create: sparse table counts"));
    GS_TRY(h->ctl.grow(1, "gs_deg_create: control words"));
    GS_TRY(dclear(h));
    GS_HIP(hipStreamSynchronize(h->stream));
    *out = guard.release();
    return GS_OK;
}

int gs_deg_destroy(gs_deg_t* h) {
    if (!h) return GS_OK;
    DeviceGuard g(h->device);
    if (h->own) (void)hipStreamSynchronize(h->own);
    if (h->stream && h->stream != h->own.get()) (void)hipStreamSynchronize(h->stream);
    delete h;
    return GS_OK;
}

int gs_deg_reset(gs_deg_t* h) {
    GS_TRY(dcheck(h, "gs_deg_reset"));
    DeviceGuard g(h->device);
    return dclear(h);
}

int gs_deg_set_stream(gs_deg_t* h, void* s) {
    GS_TRY(dcheck(h, "gs_deg_set_stream"));
    h->stream = static_cast<hipStream_t>(s);
    return GS_OK;
}

int gs_deg_get_stream(gs_deg_t* h, void** s) {
    GS_TRY(dcheck(h, "gs_deg_get_stream"));
    if (!s) return fail(GS_ERR_INVALID, "gs_deg_get_stream: null out");
    *s = h->stream;
    return GS_OK;
}

int gs_deg_sync(gs_deg_t* h) {
    GS_TRY(dcheck(h, "gs_deg_sync"));
    DeviceGuard g(h->device);
    GS_HIP(hipStreamSynchronize(h->stream));
    return GS_OK;
}

int gs_deg_fold_window(gs_deg_t* h, const void* src, const void* dst, const uint8_t* add, uint64_t n) {
    GS_TRY(dcheck(h, "gs_deg_fold_window"));
    if (n && (!src || !dst)) return fail(GS_ERR_INVALID, "gs_deg_fold_window: null edge buffer");
    return dfold(h, "gs_deg_fold_window", src, dst, add, n, std::max<uint64_t>(n, 1), nullptr, 1);
}

int gs_deg_fold_windows(gs_deg_t* h, const void* src, const void* dst, const uint8_t* add, uint64_t n, uint64_t window_edges,
                        gs_deg_window_stats* stats, uint64_t cap, uint64_t* n_windows) {
    GS_TRY(dcheck(h, "gs_deg_fold_windows"));
    if (!n_windows) return fail(GS_ERR_INVALID, "gs_deg_fold_windows: null n_windows");
    if (window_edges == 0) return fail(GS_ERR_INVALID, "gs_deg_fold_windows: window_edges is 0");
    *n_windows = 0;
    if (n == 0) return GS_OK;
    if (!src || !dst) return fail(GS_ERR_INVALID, "gs_deg_fold_windows: null edge buffer");
    const uint64_t nw = (n + window_edges - 1) / window_edges;
    *n_windows = nw;
    if (cap < nw) return fail(GS_ERR_CAPACITY, "gs_deg_fold_windows: %llu windows, capacity %llu", (unsigned long long)nw,
                              (unsigned long long)cap);
    if (!stats) return fail(GS_ERR_INVALID, "gs_deg_fold_windows: null stats");
    return dfold(h, "gs_deg_fold_windows", src, dst, add, n, window_edges, stats, nw);
}

int gs_deg_stats(gs_deg_t* h, gs_deg_window_stats* stats) {
    GS_TRY(dcheck(h, "gs_deg_stats"));
    if (!stats) return fail(GS_ERR_INVALID, "gs_deg_stats: null stats");
    DeviceGuard g(h->device);
    DegCtl c;
    GS_TRY(dread(h, c));
    stats->n_vertices = c.n_vertices;
    stats->n_degrees = c.n_degrees;
    stats->max_degree = c.maxdeg;
    stats->checksum = c.checksum;
    return GS_OK;
}

int gs_deg_path_counts(gs_deg_t* h, uint64_t* windows, uint64_t* exact_windows, uint64_t* vertex_events, uint64_t* exact_events) {
    GS_TRY(dcheck(h, "gs_deg_path_counts"));
    if (windows) *windows = h->path[0];
    if (exact_windows) *exact_windows = h->path[1];
    if (vertex_events) *vertex_events = h->path[2];
    if (exact_events) *exact_events = h->path[3];
    return GS_OK;
}

int gs_deg_emit_degrees(gs_deg_t* h, void* vertices, uint32_t* degrees, uint64_t cap, uint64_t* n_out) {
    return demit_degrees(h, "gs_deg_emit_degrees", false, vertices, degrees, cap, n_out);
}

int gs_deg_emit_degrees_delta(gs_deg_t* h, void* vertices, uint32_t* degrees, uint64_t cap, uint64_t* n_out) {
    return demit_degrees(h, "gs_deg_emit_degrees_delta", true, vertices, degrees, cap, n_out);
}

int gs_deg_emit_distribution(gs_deg_t* h, uint32_t* degrees, uint64_t* counts, uint64_t cap, uint64_t* n_out) {
    return demit_dist(h, "gs_deg_emit_distribution", 0, degrees, counts, cap, n_out);
}

int gs_deg_emit_distribution_delta(gs_deg_t* h, uint32_t* degrees, uint64_t* counts, uint64_t cap, uint64_t* n_out) {
    return demit_dist(h, "gs_deg_emit_distribution_delta", 1, degrees, counts, cap, n_out);
}

int gs_deg_find(gs_deg_t* h, const void* ids, uint32_t* degrees, uint64_t n) {
    GS_TRY(dcheck(h, "gs_deg_find"));
    if (n == 0) return GS_OK;
    if (!ids || !degrees) return fail(GS_ERR_INVALID, "gs_deg_find: null buffer");
    DeviceGuard dg(h->device);
    const size_t esz = h->id_bits / 8;
    GS_TRY(h->ebuf.grow(std::max<size_t>((size_t)h->cap * 8, dup256(n * esz) + n * 4), "degree lookup", h->stream));
    char* p = static_cast<char*>(h->ebuf.get());
    uint32_t* out = reinterpret_cast<uint32_t*>(p + dup256(n * esz));
    GS_HIP(hipMemcpyAsync(p, ids, n * esz, hipMemcpyDefault, h->stream));
    const DegArgs g = dargs(h);
    if (h->id_bits == 32)
        hipLaunchKernelGGL(k_deg_find<uint32_t>, dim3(dgrid(n)), dim3(kDegThreads), 0, h->stream, (const uint32_t*)p, out, n, g);
    else
        hipLaunchKernelGGL(k_deg_find<int64_t>, dim3(dgrid(n)), dim3(kDegThreads), 0, h->stream, (const int64_t*)p, out, n, g);
    GS_HIP(hipGetLastError());
    GS_HIP(hipMemcpyAsync(degrees, out, n * 4, hipMemcpyDefault, h->stream));
    GS_HIP(hipStreamSynchronize(h->stream));
    return GS_OK;
}

int gs_deg_restore(gs_deg_t* h, const void* vertices, const uint32_t* degrees, uint64_t n) {
    GS_TRY(dcheck(h, "gs_deg_restore"));
    if (n && (!vertices || !degrees)) return fail(GS_ERR_INVALID, "gs_deg_restore: null buffer");
    if (n > h->cap) return fail(GS_ERR_INVALID, "gs_deg_restore: %llu entries for %llu vertices (a vertex is repeated)",
                                (unsigned long long)n, (unsigned long long)h->cap);
    DeviceGuard dg(h->device);
    const size_t esz = h->id_bits / 8;
    const uint32_t m = (uint32_t)n;
    GS_TRY(h->ebuf.grow(std::max<size_t>((size_t)h->cap * 8, dup256(n * esz) + n * 4 + 256), "degree restore", h->stream));
    char* pv = static_cast<char*>(h->ebuf.get());
    uint32_t* pd = reinterpret_cast<uint32_t*>(pv + dup256(n * esz));
    const DegArgs g = dargs(h);
    const dim3 grid(dgrid(n)), block(kDegThreads);
    DegCtl c{};
    if (n) {
        GS_HIP(hipMemcpyAsync(pv, vertices, n * esz, hipMemcpyDefault, h->stream));
        GS_HIP(hipMemcpyAsync(pd, degrees, n * 4, hipMemcpyDefault, h->stream));
        GS_HIP(hipMemsetAsync(&h->ctl.get()->range, 0, 2 * sizeof(uint32_t), h->stream));
        GS_HIP(hipMemsetAsync(&h->ctl.get()->bad_zero, 0, 3 * sizeof(uint32_t), h->stream));   // bad_zero, bad_dup, vmax
        GS_HIP(hipMemsetAsync(&h->ctl.get()->vsum, 0, 8, h->stream));
        if (h->id_bits == 32) {
            hipLaunchKernelGGL(k_deg_restore_check<uint32_t>, grid, block, 0, h->stream, (const uint32_t*)pv, (const uint32_t*)pd, m, g);
            hipLaunchKernelGGL(k_deg_restore_bits<uint32_t>, grid, block, 0, h->stream, (const uint32_t*)pv, m, g);
        } else {
            hipLaunchKernelGGL(k_deg_restore_check<int64_t>, grid, block, 0, h->stream, (const int64_t*)pv, (const uint32_t*)pd, m, g);
            hipLaunchKernelGGL(k_deg_restore_bits<int64_t>, grid, block, 0, h->stream, (const int64_t*)pv, m, g);
        }
        GS_HIP(hipGetLastError());
        GS_TRY(dread(h, c));
        if (c.range) return fail(GS_ERR_RANGE, "gs_deg_restore: a vertex id outside [0, %llu)", (unsigned long long)h->cap);
        if (c.bad_zero) return fail(GS_ERR_INVALID, "gs_deg_restore: a degree of 0");
        if (c.bad_dup) return fail(GS_ERR_INVALID, "gs_deg_restore: a vertex is repeated");
        long double k = std::min<long double>((long double)h->cap, (long double)c.vsum / (long double)h->D);
        k = std::min<long double>(k, std::sqrt((double)(2.0L * (long double)c.vsum)) + 1.0L);
        if (k > (long double)(h->tcap / 4))
            return fail(GS_ERR_CAPACITY, "gs_deg_restore: more than %u distinct degrees >= %u are possible", h->tcap / 4, h->D);
    }
    GS_TRY(dclear(h));
    if (n) {
        if (h->id_bits == 32)
            hipLaunchKernelGGL(k_deg_restore_apply<uint32_t>, grid, block, 0, h->stream, (const uint32_t*)pv, (const uint32_t*)pd, m, g);
        else
            hipLaunchKernelGGL(k_deg_restore_apply<int64_t>, grid, block, 0, h->stream, (const int64_t*)pv, (const uint32_t*)pd, m, g);
        hipLaunchKernelGGL(k_deg_finish, dim3(1), dim3(1), 0, h->stream, g, (unsigned long long*)nullptr);
        hipLaunchKernelGGL(k_deg_snapshot, dim3(dgrid((uint64_t)h->D + h->tcap)), block, 0, h->stream, g);
        GS_HIP(hipGetLastError());
        GS_HIP(hipStreamSynchronize(h->stream));
    }
    h->restored_max = c.vmax;
    h->sum_bound = (long double)c.vsum;
    return GS_OK;
}

}  // extern "C"
