// slice.hip — neighbourhood slices on the device: the reference's SimpleEdgeStream.slice(size,
// direction) -> SnapshotStream (SimpleEdgeStream.java:135-167) with reduceOnEdges / foldNeighbors /
// applyOnNeighbors (SnapshotStream.java:61-131), extern "C" in include/gsgpu.h (gs_slice_*).
//
// A window of n edges (s, d, x) becomes entries (key, neighbour, value): OUT (s, d, x), IN (d, s, x),
// ALL both, (s, d, x) at position 2i and (d, s, x) at 2i + 1. The row of a vertex is its entries in
// arrival order. Everything runs on the handle's stream, with no host wait inside a window or
// between the windows of a multi-window call:
//   1 keys     ids range-checked; per entry its key vertex, its neighbour and its position
//   2 sort     hipcub SortPairs (key -> position) over the bits the capacity needs. The sort is
//              stable, so a row's positions ascend: arrival order, with no position in the key.
//   3 rows     heads = entries whose sorted key differs from the predecessor's; an inclusive scan of
//              the heads numbers the rows (rid, 1-based). Row r's vertex and start are written by
//              its head; the last entry writes the end sentinel and the row count nv, which stays in
//              device memory for the kernels that follow.
//   4 reduce   SUM / MIN / MAX, k_slice_reduce: work is split over ENTRIES, kSliceTile per workgroup,
//              so a hub row costs what its entries cost. A wave takes 64 consecutive sorted entries,
//              gathers their values through the sorted positions and scans them segmented by row
//              through shuffles. A row that lies inside the wave is stored by its last lane. A row
//              that crosses a wave boundary leaves a partial in LDS (at most two per wave: its first
//              and its last row); one wave combines the workgroup's partials with the same scan and
//              sends one 64-bit atomic per row onto a slot pre-set to the op's identity. No atomic
//              per entry. COUNT / FIRST / LAST come from the row bounds and one gather.
//   5 CSR      neighbours and values gathered into sorted order, ids widened to id_bits
//   6 stats    rows, entries, longest row, checksum over (vertex, reduced value)
// No array here is indexed by vertex id, so there is nothing of O(capacity) to allocate or to clear
// between windows: all state is O(entries) and overwritten by the next window.
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstring>
#include <memory>

#include <hipcub/hipcub.hpp>

#include "owned.hpp"

namespace gsgpu {

constexpr uint32_t kSliceThreads = 256;
constexpr uint32_t kSliceWaves = kSliceThreads / 64;
constexpr uint32_t kSliceItems = 8;                               // entries per lane in k_slice_reduce
constexpr uint32_t kSliceTile = kSliceThreads * kSliceItems;      // entries per workgroup there
constexpr uint32_t kSliceSlots = 2 * kSliceWaves * kSliceItems;   // partials per workgroup: one wave's worth
constexpr unsigned kSliceMaxBlocks = 4096;
static_assert(kSliceSlots == 64, "one wave combines the workgroup's partials, a slot per lane");

// control words of a call, in device memory
struct SliceCtl {
    uint32_t nv;                              // rows of the window last built
    uint32_t range;                           // an id outside [0, capacity) was seen (kept for the call)
    uint32_t overflow;                        // the records of a multi-window call outgrew the capacity
    uint32_t pad;
};

// What the sort carries next to an entry's key. The product carries the entry's position and
// gathers the value through it afterwards; the experiment build GS_EXP_SLICE_PAYLOAD (make exp)
// carries the value through the sort as well, for the comparison of DESIGN.md section 4f.
struct SliceEntry {
    long long val;
    uint32_t pos, pad;
};
#ifdef GS_EXP_SLICE_PAYLOAD
using SlicePos = SliceEntry;
#else
using SlicePos = uint32_t;
#endif
__device__ __forceinline__ uint32_t slice_pos(const uint32_t* p, uint32_t i) { return p[i]; }
__device__ __forceinline__ uint32_t slice_pos(const SliceEntry* p, uint32_t i) { return p[i].pos; }
__device__ __forceinline__ long long slice_val(const uint32_t* p, uint32_t i, const long long* val, uint32_t shift) {
    return val[p[i] >> shift];
}
__device__ __forceinline__ long long slice_val(const SliceEntry* p, uint32_t i, const long long*, uint32_t) { return p[i].val; }
__device__ __forceinline__ void slice_put(uint32_t* p, uint32_t j, const long long*, uint32_t) { p[j] = j; }
__device__ __forceinline__ void slice_put(SliceEntry* p, uint32_t j, const long long* val, uint32_t e) {
    p[j] = SliceEntry{val ? val[e] : 0ll, j, 0u};
}

// step 1 (val: the window's values, already on the device; null for a slice without values)
template <typename IdT>
__global__ __launch_bounds__(kSliceThreads) void k_slice_keys(const IdT* __restrict__ src, const IdT* __restrict__ dst,
                                                              uint32_t n, uint32_t dir, uint64_t cap,
                                                              uint32_t* __restrict__ keys, SlicePos* __restrict__ pos,
                                                              const long long* __restrict__ val,
                                                              uint32_t* __restrict__ nb, SliceCtl* __restrict__ ctl) {
    bool bad = false;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const IdT x = src[i], y = dst[i];
        const bool ok = (uint64_t)x < cap && (uint64_t)y < cap;         // (a negative int64 is >= 2^63)
        bad |= !ok;
        const uint32_t u = ok ? (uint32_t)x : 0u, v = ok ? (uint32_t)y : 0u;
        if (dir == GS_SLICE_ALL) {
            reinterpret_cast<uint2*>(keys)[i] = make_uint2(u, v);
            reinterpret_cast<uint2*>(nb)[i] = make_uint2(v, u);
            slice_put(pos, 2 * i, val, i);
            slice_put(pos, 2 * i + 1, val, i);
        } else {
            keys[i] = dir == GS_SLICE_OUT ? u : v;
            nb[i] = dir == GS_SLICE_OUT ? v : u;
            slice_put(pos, i, val, i);
        }
    }
    if (bad) atomicOr(&ctl->range, 1u);
}

// step 3
__global__ __launch_bounds__(kSliceThreads) void k_slice_heads(const uint32_t* __restrict__ keys, uint32_t ne,
                                                               uint32_t* __restrict__ heads) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < ne; i += gridDim.x * blockDim.x)
        heads[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// rid = the inclusive scan of the heads: entry i lies in row rid[i] - 1
__global__ __launch_bounds__(kSliceThreads) void k_slice_rows(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ rid,
                                                              uint32_t ne, uint32_t* __restrict__ rv, uint32_t* __restrict__ rs,
                                                              SliceCtl* __restrict__ ctl) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < ne; i += gridDim.x * blockDim.x) {
        const uint32_t r = rid[i];
        if (i == 0 || rid[i - 1] != r) {
            rv[r - 1] = keys[i];
            rs[r - 1] = i;
        }
        if (i + 1 == ne) {
            rs[r] = ne;
            ctl->nv = r;
        }
    }
}

// step 4
template <int OP> __device__ __forceinline__ long long slice_identity() {
    return OP == GS_SLICE_MIN ? LLONG_MAX : OP == GS_SLICE_MAX ? LLONG_MIN : 0ll;
}
template <int OP> __device__ __forceinline__ long long slice_op(long long a, long long b) {
    if (OP == GS_SLICE_MIN) return a < b ? a : b;
    if (OP == GS_SLICE_MAX) return a > b ? a : b;
    return (long long)((unsigned long long)a + (unsigned long long)b);     // wraps as Java long
}
template <int OP> __device__ __forceinline__ void slice_atomic(long long* p, long long v) {
    if (OP == GS_SLICE_MIN) atomicMin(p, v);
    else if (OP == GS_SLICE_MAX) atomicMax(p, v);
    else atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// inclusive scan of v over the wave, restarted where r changes (equal r are contiguous)
template <int OP> __device__ __forceinline__ long long slice_seg_scan(long long v, uint32_t r, uint32_t lane) {
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const long long t = __shfl_up(v, off, 64);
        const uint32_t rr = __shfl_up(r, off, 64);
        if (lane >= off && rr == r) v = slice_op<OP>(t, v);
    }
    return v;
}

template <int OP>
__global__ __launch_bounds__(kSliceThreads) void k_slice_fill(long long* __restrict__ out, const SliceCtl* __restrict__ ctl) {
    const uint32_t nv = ctl->nv;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < nv; r += gridDim.x * blockDim.x) out[r] = slice_identity<OP>();
}

// One workgroup per tile of kSliceTile sorted entries; shift = 1 under ALL (two entries per edge).
template <int OP>
__global__ __launch_bounds__(kSliceThreads) void k_slice_reduce(const uint32_t* __restrict__ rid, const SlicePos* __restrict__ pos,
                                                                const long long* __restrict__ val, uint32_t ne, uint32_t shift,
                                                                long long* __restrict__ out) {
    __shared__ uint32_t srow[kSliceSlots];
    __shared__ long long sval[kSliceSlots];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t base = blockIdx.x * kSliceTile;
#pragma unroll 2
    for (uint32_t k = 0; k < kSliceItems; ++k) {
        const uint32_t i = base + k * kSliceThreads + threadIdx.x;
        const bool in = i < ne;
        const uint32_t r = in ? rid[i] : kInvalid;                          // (rows are numbered from 1)
        long long v = in ? slice_val(pos, i, val, shift) : slice_identity<OP>();
        uint32_t rprev = __shfl_up(r, 1, 64), rnext = __shfl_down(r, 1, 64);
        if (lane == 0) rprev = (in && i > 0) ? rid[i - 1] : kInvalid;
        if (lane == 63) rnext = (in && i + 1 < ne) ? rid[i + 1] : kInvalid;
        const bool head = in && (i == 0 || r != rprev), tail = in && r != rnext;
        v = slice_seg_scan<OP>(v, r, lane);
        const uint32_t r0 = __shfl(r, 0, 64), r63 = __shfl(r, 63, 64);
        const bool head0 = __shfl((int)head, 0, 64) != 0;
        const unsigned long long tails = __ballot(tail);
        // a row with its head and its tail in this wave is complete
        if (tail && (r != r0 || head0)) out[r - 1] = v;
        // the partials: the wave's first row when its head lies before the wave (or the whole wave
        // is one row that goes on), and its last row when it goes on into the next wave
        const uint32_t t0 = tails ? (uint32_t)__ffsll((long long)tails) - 1 : 63u;
        const long long v0 = __shfl(v, (int)t0, 64), v63 = __shfl(v, 63, 64);
        if (lane == 0) {
            const uint32_t s = 2 * (k * kSliceWaves + wave);
            const bool first = r0 != kInvalid && (tails == 0 || !head0);
            const bool last = tails != 0 && r63 != kInvalid && !((tails >> 63) & 1ull);
            srow[s] = first ? r0 : kInvalid;
            sval[s] = first ? v0 : slice_identity<OP>();
            srow[s + 1] = last ? r63 : kInvalid;
            sval[s + 1] = last ? v63 : slice_identity<OP>();
        }
    }
    __syncthreads();
    if (wave != 0) return;
    // the slots are in entry order; an empty slot joins the row before it with the identity, so a
    // row's partials form one run and the row gets one atomic from this workgroup
    uint32_t r = srow[lane];
    long long v = sval[lane];
    const unsigned long long valid = __ballot(r != kInvalid);
    const unsigned long long upto = valid & ((2ull << lane) - 1);            // (lane 63: 2 << 63 wraps to 0, - 1 = all)
    const int p = upto ? 63 - __clzll((long long)upto) : 0;
    const uint32_t rfill = __shfl(r, p, 64);
    r = upto ? rfill : kInvalid;
    v = slice_seg_scan<OP>(v, r, lane);
    const uint32_t rnext = __shfl_down(r, 1, 64);
    if (r != kInvalid && (lane == 63 || r != rnext)) slice_atomic<OP>(&out[r - 1], v);
}

// COUNT / FIRST / LAST: the row bounds and one gather
template <int OP>
__global__ __launch_bounds__(kSliceThreads) void k_slice_bounds(const uint32_t* __restrict__ rs, const SlicePos* __restrict__ pos,
                                                                const long long* __restrict__ val, uint32_t shift,
                                                                long long* __restrict__ out, const SliceCtl* __restrict__ ctl) {
    const uint32_t nv = ctl->nv;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < nv; r += gridDim.x * blockDim.x) {
        const uint32_t a = rs[r], b = rs[r + 1];
        out[r] = OP == GS_SLICE_COUNT ? (long long)(b - a) : slice_val(pos, OP == GS_SLICE_FIRST ? a : b - 1, val, shift);
    }
}

// step 5
template <typename IdT>
__global__ __launch_bounds__(kSliceThreads) void k_slice_widen(const uint32_t* __restrict__ in, IdT* __restrict__ out, uint32_t n) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = (IdT)in[i];
}

// (values may be null: a slice without values)
template <typename IdT>
__global__ __launch_bounds__(kSliceThreads) void k_slice_csr(const SlicePos* __restrict__ pos, const uint32_t* __restrict__ nb,
                                                             const long long* __restrict__ val, uint32_t ne, uint32_t shift,
                                                             IdT* __restrict__ neighbours, long long* __restrict__ values) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < ne; i += gridDim.x * blockDim.x) {
        neighbours[i] = (IdT)nb[slice_pos(pos, i)];
        if (values) values[i] = slice_val(pos, i, val, shift);
    }
}

// step 6; *st is zero when the kernel starts
__global__ __launch_bounds__(kSliceThreads) void k_slice_stats(const uint32_t* __restrict__ rv, const uint32_t* __restrict__ rs,
                                                               const long long* __restrict__ red, uint32_t ne,
                                                               const SliceCtl* __restrict__ ctl, gs_slice_window_stats* __restrict__ st) {
    if (ctl->range) return;
    const uint32_t nv = ctl->nv;
    unsigned long long sum = 0, mx = 0;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < nv; r += gridDim.x * blockDim.x) {
        sum += pair_mix(rv[r], (uint64_t)red[r]);
        mx = max(mx, (unsigned long long)(rs[r + 1] - rs[r]));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_down(sum, off, 64);
        mx = max(mx, (unsigned long long)__shfl_down(mx, off, 64));
    }
    if ((threadIdx.x & 63) == 0 && mx) {
        atomicAdd(reinterpret_cast<unsigned long long*>(&st->checksum), sum);
        atomicMax(reinterpret_cast<unsigned long long*>(&st->max_row), mx);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->n_vertices = nv;
        st->n_entries = ne;
    }
}

// a multi-window call: window w's records go behind those of the windows before it
template <typename IdT>
__global__ __launch_bounds__(kSliceThreads) void k_slice_append(const uint32_t* __restrict__ rv, const long long* __restrict__ red,
                                                                SliceCtl* __restrict__ ctl, unsigned long long* __restrict__ woff,
                                                                uint32_t w, IdT* __restrict__ vertices, long long* __restrict__ values,
                                                                uint64_t cap) {
    const bool range = ctl->range != 0;
    const uint32_t nv = range ? 0u : ctl->nv;
    const unsigned long long start = woff[w];
    const bool fits = start + nv <= cap;
    if (fits)
        for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < nv; r += gridDim.x * blockDim.x) {
            vertices[start + r] = (IdT)rv[r];
            values[start + r] = red[r];
        }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        woff[w + 1] = start + nv;
        if (!fits) ctl->overflow = 1;
    }
}

}  // namespace gsgpu

using namespace gsgpu;

namespace {

// the layout of a window's slice in the handle's scratch, for windows of up to n edges
struct SliceScratch {
    long long* val = nullptr;                  // [n] the edge values
    uint32_t* nb = nullptr;                    // [ne] neighbour per entry, in arrival order
    uint32_t *ka = nullptr, *kb = nullptr;     // [ne] keys: unsorted (then the heads), sorted
    SlicePos *pa = nullptr, *pb = nullptr;     // [ne] positions: unsorted, sorted
    uint32_t* rid = nullptr;                   // [ne] row number per sorted entry (over pa, which the sort has consumed)
    uint32_t *rv = nullptr, *rs = nullptr;     // [ne], [ne + 1] row vertex, row start
    long long* red = nullptr;                  // [ne] a reduction, one value per row
    void* tmp = nullptr;                       // hipcub's temporaries
    size_t sort_bytes = 0, scan_bytes = 0;
};

}  // namespace

struct gs_slice {
    uint64_t cap = 0;
    uint32_t id_bits = 64, bits = 1, dir = GS_SLICE_OUT;
    int device = 0;
    Stream own;
    hipStream_t stream = nullptr;              // own, or the caller's (gs_slice_set_stream)
    DevBuf<SliceCtl> ctl;
    DevBuf<> tmp;                              // the slice and its scratch: by the largest window seen
    DevBuf<> stage;                            // host src / dst of one window
    DevBuf<> ebuf;                             // emission: widened ids, CSR arrays, records for host arrays
    DevBuf<unsigned long long> woff;           // window offsets of a multi-window call
    DevBuf<gs_slice_window_stats> dstats;      // per-window statistics
    Pinned<> hbuf;                             // pinned mirror of ctl, woff, dstats
    size_t hbuf_cap = 0;
    SliceScratch s;
    // the slice held: edges, entries, rows, and whether it has values
    uint64_t n = 0, ne = 0, nv = 0;
    bool has_val = false;
};

namespace {

constexpr uint64_t kSliceMaxCap = 1ull << 32;
constexpr uint64_t kSliceMaxWindow = (1ull << 30) - 1;

int scheck(gs_slice_t* h, const char* fn) { return h ? GS_OK : fail(GS_ERR_INVALID, "%s: null handle", fn); }

unsigned sgrid(uint64_t items) {
    const uint64_t b = (items + kSliceThreads - 1) / kSliceThreads;
    return (unsigned)std::min<uint64_t>(std::max<uint64_t>(b, 1), kSliceMaxBlocks);
}

size_t sup256(size_t x) { return (x + 255) & ~(size_t)255; }

bool sop_ok(int op) { return op >= GS_SLICE_SUM && op <= GS_SLICE_LAST; }

uint64_t sentries(const gs_slice_t* h, uint64_t n) { return h->dir == GS_SLICE_ALL ? 2 * n : n; }

int spinned(gs_slice_t* h, size_t bytes) {
    if (h->hbuf_cap >= bytes) return GS_OK;
    GS_TRY(h->hbuf.alloc(bytes, "slice read-back"));
    h->hbuf_cap = bytes;
    return GS_OK;
}

int sscratch(gs_slice_t* h, uint64_t n) {
    SliceScratch& s = h->s;
    const uint64_t ne = sentries(h, n);
    GS_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, s.sort_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                              (const SlicePos*)nullptr, (SlicePos*)nullptr, (int)ne, 0, (int)h->bits, h->stream));
    GS_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, s.scan_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)ne, h->stream));
    const size_t vbytes = sup256(n * 8), ebytes = sup256(ne * 4 + 4), rbytes = sup256(ne * 8);
    const size_t pbytes = sup256(ne * sizeof(SlicePos)), tbytes = sup256(std::max(s.sort_bytes, s.scan_bytes));
    GS_TRY(h->tmp.grow(vbytes + 5 * ebytes + 2 * pbytes + rbytes + tbytes, "slice scratch", h->stream));
    char* p = static_cast<char*>(h->tmp.get());
    s.val = reinterpret_cast<long long*>(p); p += vbytes;
    uint32_t** words[] = {&s.nb, &s.ka, &s.kb, &s.rv, &s.rs};
    for (uint32_t** w : words) { *w = reinterpret_cast<uint32_t*>(p); p += ebytes; }
    s.pa = reinterpret_cast<SlicePos*>(p); p += pbytes;
    s.pb = reinterpret_cast<SlicePos*>(p); p += pbytes;
    s.rid = reinterpret_cast<uint32_t*>(s.pa);
    s.red = reinterpret_cast<long long*>(p); p += rbytes;
    s.tmp = p;
    return GS_OK;
}

// Steps 1 to 3 for one window of n edges (n >= 1), the values copied next to it; enqueues only.
int sbuild(gs_slice_t* h, const void* src, const void* dst, const int64_t* val, uint64_t off, uint32_t n, bool dev) {
    const SliceScratch& s = h->s;
    const size_t esz = h->id_bits / 8;
    const void *a = static_cast<const char*>(src) + off * esz, *b = static_cast<const char*>(dst) + off * esz;
    if (!dev) {
        char* s0 = static_cast<char*>(h->stage.get());
        char* s1 = s0 + sup256(n * esz);
        GS_HIP(hipMemcpyAsync(s0, a, n * esz, hipMemcpyDefault, h->stream));
        GS_HIP(hipMemcpyAsync(s1, b, n * esz, hipMemcpyDefault, h->stream));
        a = s0;
        b = s1;
    }
    if (val) GS_HIP(hipMemcpyAsync(s.val, val + off, (size_t)n * 8, hipMemcpyDefault, h->stream));
    const uint32_t ne = (uint32_t)sentries(h, n);
    const dim3 block(kSliceThreads);
    if (h->id_bits == 32)
        hipLaunchKernelGGL(k_slice_keys<uint32_t>, dim3(sgrid(n)), block, 0, h->stream, (const uint32_t*)a, (const uint32_t*)b, n,
                           h->dir, h->cap, s.ka, s.pa, val ? (const long long*)s.val : nullptr, s.nb, h->ctl.get());
    else
        hipLaunchKernelGGL(k_slice_keys<int64_t>, dim3(sgrid(n)), block, 0, h->stream, (const int64_t*)a, (const int64_t*)b, n,
                           h->dir, h->cap, s.ka, s.pa, val ? (const long long*)s.val : nullptr, s.nb, h->ctl.get());
    GS_HIP(hipGetLastError());
    size_t bytes = s.sort_bytes;
    GS_HIP(hipcub::DeviceRadixSort::SortPairs(s.tmp, bytes, (const uint32_t*)s.ka, s.kb, (const SlicePos*)s.pa, s.pb, (int)ne, 0,
                                              (int)h->bits, h->stream));
    hipLaunchKernelGGL(k_slice_heads, dim3(sgrid(ne)), block, 0, h->stream, (const uint32_t*)s.kb, ne, s.ka);
    GS_HIP(hipGetLastError());
    bytes = s.scan_bytes;
    GS_HIP(hipcub::DeviceScan::InclusiveSum(s.tmp, bytes, (const uint32_t*)s.ka, s.rid, (int)ne, h->stream));
    hipLaunchKernelGGL(k_slice_rows, dim3(sgrid(ne)), block, 0, h->stream, (const uint32_t*)s.kb, (const uint32_t*)s.rid, ne, s.rv,
                       s.rs, h->ctl.get());
    GS_HIP(hipGetLastError());
    return GS_OK;
}

template <int OP>
void sreduce_op(gs_slice_t* h, uint32_t ne) {
    const SliceScratch& s = h->s;
    const uint32_t shift = h->dir == GS_SLICE_ALL ? 1 : 0;
    const dim3 block(kSliceThreads);
    if constexpr (OP == GS_SLICE_SUM || OP == GS_SLICE_MIN || OP == GS_SLICE_MAX) {
        hipLaunchKernelGGL(k_slice_fill<OP>, dim3(sgrid(ne)), block, 0, h->stream, s.red, (const SliceCtl*)h->ctl.get());
        hipLaunchKernelGGL(k_slice_reduce<OP>, dim3((ne + kSliceTile - 1) / kSliceTile), block, 0, h->stream, (const uint32_t*)s.rid,
                           (const SlicePos*)s.pb, (const long long*)s.val, ne, shift, s.red);
    } else {
        hipLaunchKernelGGL(k_slice_bounds<OP>, dim3(sgrid(ne)), block, 0, h->stream, (const uint32_t*)s.rs, (const SlicePos*)s.pb,
                           (const long long*)s.val, shift, s.red, (const SliceCtl*)h->ctl.get());
    }
}

// step 4 for the slice in the scratch (ne >= 1): one value per row into s.red; enqueues only
int sreduce(gs_slice_t* h, int op, uint32_t ne) {
    switch (op) {
        case GS_SLICE_SUM: sreduce_op<GS_SLICE_SUM>(h, ne); break;
        case GS_SLICE_MIN: sreduce_op<GS_SLICE_MIN>(h, ne); break;
        case GS_SLICE_MAX: sreduce_op<GS_SLICE_MAX>(h, ne); break;
        case GS_SLICE_COUNT: sreduce_op<GS_SLICE_COUNT>(h, ne); break;
        case GS_SLICE_FIRST: sreduce_op<GS_SLICE_FIRST>(h, ne); break;
        default: sreduce_op<GS_SLICE_LAST>(h, ne); break;
    }
    GS_HIP(hipGetLastError());
    return GS_OK;
}

int sstats(gs_slice_t* h, uint32_t ne, gs_slice_window_stats* st) {
    const SliceScratch& s = h->s;
    hipLaunchKernelGGL(k_slice_stats, dim3(sgrid(ne)), dim3(kSliceThreads), 0, h->stream, (const uint32_t*)s.rv, (const uint32_t*)s.rs,
                       (const long long*)s.red, ne, (const SliceCtl*)h->ctl.get(), st);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

// what a reduction or an emission needs of the slice held
int sready(gs_slice_t* h, const char* fn, int op) {
    if (!sop_ok(op)) return fail(GS_ERR_INVALID, "%s: unknown op %d", fn, op);
    if (op != GS_SLICE_COUNT && h->ne && !h->has_val)
        return fail(GS_ERR_INVALID, "%s: the slice was built without values; only GS_SLICE_COUNT applies", fn);
    return GS_OK;
}

// n ids of the slice (32-bit words on the device) into a host or device array id_bits wide; enqueues only
int sids_out(gs_slice_t* h, const uint32_t* in, uint64_t n, void* out, void* wide) {
    if (h->id_bits == 32) {
        GS_HIP(hipMemcpyAsync(out, in, n * 4, hipMemcpyDefault, h->stream));
        return GS_OK;
    }
    int64_t* w = is_device_pointer(out) ? static_cast<int64_t*>(out) : static_cast<int64_t*>(wide);
    hipLaunchKernelGGL(k_slice_widen<int64_t>, dim3(sgrid(n)), dim3(kSliceThreads), 0, h->stream, in, w, (uint32_t)n);
    GS_HIP(hipGetLastError());
    if (w != out) GS_HIP(hipMemcpyAsync(out, w, n * 8, hipMemcpyDefault, h->stream));
    return GS_OK;
}

}  // namespace

extern "C" {

int gs_slice_create(gs_slice_t** out, uint64_t vertex_capacity, uint32_t id_bits, int device, uint32_t direction) {
    if (!out) return fail(GS_ERR_INVALID, "gs_slice_create: null out");
    *out = nullptr;
    if (direction > GS_SLICE_ALL) return fail(GS_ERR_INVALID, "gs_slice_create: unknown direction %u", direction);
    if (id_bits != 32 && id_bits != 64) return fail(GS_ERR_INVALID, "gs_slice_create: id_bits must be 32 or 64");
    if (vertex_capacity == 0 || vertex_capacity > kSliceMaxCap)
        return fail(GS_ERR_INVALID, "gs_slice_create: vertex_capacity must be in [1, 2^32]");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return fail(GS_ERR_HIP, "gs_slice_create: no HIP device available");
    }
    if (device < 0 || device >= ndev) return fail(GS_ERR_INVALID, "gs_slice_create: device %d of %d", device, ndev);
    DeviceGuard g(device);
    gs_slice_t* h = new gs_slice_t();
    struct Destroy { void operator()(gs_slice_t* p) const { (void)gs_slice_destroy(p); } };
    std::unique_ptr<gs_slice_t, Destroy> guard(h);    // a failure below destroys what exists so far
    h->cap = vertex_capacity;
    h->id_bits = id_bits;
    h->dir = direction;
    h->device = device;
    while (h->bits < 32 && (1ull << h->bits) < vertex_capacity) ++h->bits;
    GS_TRY(h->own.create());
    h->stream = h->own;
    GS_TRY(h->ctl.grow(1, "gs_slice_create: control words"));
    GS_HIP(hipMemsetAsync(h->ctl.get(), 0, sizeof(SliceCtl), h->stream));
    GS_HIP(hipStreamSynchronize(h->stream));
    *out = guard.release();
    return GS_OK;
}

int gs_slice_destroy(gs_slice_t* h) {
    if (!h) return GS_OK;
    DeviceGuard g(h->device);
    if (h->own) (void)hipStreamSynchronize(h->own);
    if (h->stream && h->stream != h->own.get()) (void)hipStreamSynchronize(h->stream);
    delete h;                                  // the owners free what it holds (owned.hpp)
    return GS_OK;
}

int gs_slice_set_stream(gs_slice_t* h, void* s) {
    GS_TRY(scheck(h, "gs_slice_set_stream"));
    h->stream = static_cast<hipStream_t>(s);
    return GS_OK;
}

int gs_slice_get_stream(gs_slice_t* h, void** s) {
    GS_TRY(scheck(h, "gs_slice_get_stream"));
    if (!s) return fail(GS_ERR_INVALID, "gs_slice_get_stream: null out");
    *s = h->stream;
    return GS_OK;
}

int gs_slice_sync(gs_slice_t* h) {
    GS_TRY(scheck(h, "gs_slice_sync"));
    DeviceGuard g(h->device);
    GS_HIP(hipStreamSynchronize(h->stream));
    return GS_OK;
}

int gs_slice_window(gs_slice_t* h, const void* src, const void* dst, const int64_t* val, uint64_t n) {
    GS_TRY(scheck(h, "gs_slice_window"));
    if (n && (!src || !dst)) return fail(GS_ERR_INVALID, "gs_slice_window: null edge buffer");
    if (n > kSliceMaxWindow) return fail(GS_ERR_UNSUPPORTED, "gs_slice_window: more than 2^30 - 1 edges");
    h->n = h->ne = h->nv = 0;
    h->has_val = val != nullptr;
    if (n == 0) return GS_OK;
    DeviceGuard g(h->device);
    const bool dev = is_device_pointer(src) && is_device_pointer(dst);
    GS_TRY(sscratch(h, n));
    if (!dev) GS_TRY(h->stage.grow(2 * sup256(n * (h->id_bits / 8)), "slice input staging", h->stream));
    GS_TRY(spinned(h, sizeof(SliceCtl)));
    GS_HIP(hipMemsetAsync(h->ctl.get(), 0, sizeof(SliceCtl), h->stream));
    GS_TRY(sbuild(h, src, dst, val, 0, (uint32_t)n, dev));
    GS_HIP(hipMemcpyAsync(h->hbuf.get(), h->ctl.get(), sizeof(SliceCtl), hipMemcpyDeviceToHost, h->stream));
    GS_HIP(hipStreamSynchronize(h->stream));
    SliceCtl c;
    memcpy(&c, h->hbuf.get(), sizeof(SliceCtl));
    if (c.range) return fail(GS_ERR_RANGE, "gs_slice_window: a vertex id outside [0, %llu); the slice is empty", (unsigned long long)h->cap);
    h->n = n;
    h->ne = sentries(h, n);
    h->nv = c.nv;
    return GS_OK;
}

int gs_slice_reduce(gs_slice_t* h, int op, void* vertices, int64_t* values, uint64_t cap, uint64_t* n_out) {
    GS_TRY(scheck(h, "gs_slice_reduce"));
    if (!n_out) return fail(GS_ERR_INVALID, "gs_slice_reduce: null n_out");
    GS_TRY(sready(h, "gs_slice_reduce", op));
    *n_out = h->nv;
    if (cap < h->nv) return fail(GS_ERR_CAPACITY, "gs_slice_reduce: %llu rows, capacity %llu", (unsigned long long)h->nv,
                                 (unsigned long long)cap);
    if (h->nv == 0) return GS_OK;
    if (!vertices || !values) return fail(GS_ERR_INVALID, "gs_slice_reduce: null output");
    DeviceGuard g(h->device);
    if (h->id_bits == 64 && !is_device_pointer(vertices)) GS_TRY(h->ebuf.grow((size_t)h->nv * 8, "slice emission", h->stream));
    GS_TRY(sreduce(h, op, (uint32_t)h->ne));
    GS_TRY(sids_out(h, h->s.rv, h->nv, vertices, h->ebuf.get()));
    GS_HIP(hipMemcpyAsync(values, h->s.red, (size_t)h->nv * 8, hipMemcpyDefault, h->stream));
    GS_HIP(hipStreamSynchronize(h->stream));
    return GS_OK;
}

int gs_slice_rows(gs_slice_t* h, void* vertices, uint64_t* offsets, void* neighbours, int64_t* values,
                  uint64_t cap_vertices, uint64_t cap_entries, uint64_t* n_vertices, uint64_t* n_entries) {
    GS_TRY(scheck(h, "gs_slice_rows"));
    if (!n_vertices || !n_entries) return fail(GS_ERR_INVALID, "gs_slice_rows: null count output");
    *n_vertices = h->nv;
    *n_entries = h->ne;
    if (values && h->ne && !h->has_val)
        return fail(GS_ERR_INVALID, "gs_slice_rows: the slice was built without values; values must be NULL");
    if (cap_vertices < h->nv || cap_entries < h->ne)
        return fail(GS_ERR_CAPACITY, "gs_slice_rows: %llu rows and %llu entries, capacities %llu and %llu", (unsigned long long)h->nv,
                    (unsigned long long)h->ne, (unsigned long long)cap_vertices, (unsigned long long)cap_entries);
    if (!offsets) return fail(GS_ERR_INVALID, "gs_slice_rows: null offsets");
    DeviceGuard g(h->device);
    if (h->nv == 0) {
        const uint64_t zero = 0;
        GS_HIP(hipMemcpyAsync(offsets, &zero, 8, hipMemcpyDefault, h->stream));
        GS_HIP(hipStreamSynchronize(h->stream));
        return GS_OK;
    }
    if (!vertices || !neighbours || (h->has_val && !values)) return fail(GS_ERR_INVALID, "gs_slice_rows: null output");
    const SliceScratch& s = h->s;
    const uint32_t nv = (uint32_t)h->nv, ne = (uint32_t)h->ne, shift = h->dir == GS_SLICE_ALL ? 1 : 0;
    const size_t isz = h->id_bits / 8;
    // emission scratch: vertices | offsets | neighbours | values, each used only for a host array
    const size_t b0 = sup256((size_t)nv * 8), b1 = sup256(((size_t)nv + 1) * 8), b2 = sup256((size_t)ne * 8);
    GS_TRY(h->ebuf.grow(b0 + b1 + 2 * b2, "slice emission", h->stream));
    char* e = static_cast<char*>(h->ebuf.get());
    const dim3 block(kSliceThreads);
    GS_TRY(sids_out(h, s.rv, nv, vertices, e));
    unsigned long long* off = is_device_pointer(offsets) ? reinterpret_cast<unsigned long long*>(offsets)
                                                         : reinterpret_cast<unsigned long long*>(e + b0);
    hipLaunchKernelGGL(k_slice_widen<unsigned long long>, dim3(sgrid(nv + 1)), block, 0, h->stream, (const uint32_t*)s.rs, off, nv + 1);
    void* nbo = is_device_pointer(neighbours) ? neighbours : static_cast<void*>(e + b0 + b1);
    long long* vo = !values ? nullptr
                            : is_device_pointer(values) ? reinterpret_cast<long long*>(values) : reinterpret_cast<long long*>(e + b0 + b1 + b2);
    if (h->id_bits == 32)
        hipLaunchKernelGGL(k_slice_csr<uint32_t>, dim3(sgrid(ne)), block, 0, h->stream, (const SlicePos*)s.pb, (const uint32_t*)s.nb,
                           (const long long*)s.val, ne, shift, static_cast<uint32_t*>(nbo), vo);
    else
        hipLaunchKernelGGL(k_slice_csr<int64_t>, dim3(sgrid(ne)), block, 0, h->stream, (const SlicePos*)s.pb, (const uint32_t*)s.nb,
                           (const long long*)s.val, ne, shift, static_cast<int64_t*>(nbo), vo);
    GS_HIP(hipGetLastError());
    if ((void*)off != (void*)offsets) GS_HIP(hipMemcpyAsync(offsets, off, ((size_t)nv + 1) * 8, hipMemcpyDefault, h->stream));
    if (nbo != neighbours) GS_HIP(hipMemcpyAsync(neighbours, nbo, (size_t)ne * isz, hipMemcpyDefault, h->stream));
    if (vo && (void*)vo != (void*)values) GS_HIP(hipMemcpyAsync(values, vo, (size_t)ne * 8, hipMemcpyDefault, h->stream));
    GS_HIP(hipStreamSynchronize(h->stream));
    return GS_OK;
}

int gs_slice_stats(gs_slice_t* h, int op, gs_slice_window_stats* stats) {
    GS_TRY(scheck(h, "gs_slice_stats"));
    if (!stats) return fail(GS_ERR_INVALID, "gs_slice_stats: null stats");
    GS_TRY(sready(h, "gs_slice_stats", op));
    memset(stats, 0, sizeof(*stats));
    if (h->ne == 0) return GS_OK;
    DeviceGuard g(h->device);
    GS_TRY(h->dstats.grow(1, "slice statistics", h->stream));
    GS_TRY(spinned(h, sizeof(gs_slice_window_stats)));
    GS_HIP(hipMemsetAsync(h->dstats.get(), 0, sizeof(gs_slice_window_stats), h->stream));
    GS_TRY(sreduce(h, op, (uint32_t)h->ne));
    GS_TRY(sstats(h, (uint32_t)h->ne, h->dstats.get()));
    GS_HIP(hipMemcpyAsync(h->hbuf.get(), h->dstats.get(), sizeof(gs_slice_window_stats), hipMemcpyDeviceToHost, h->stream));
    GS_HIP(hipStreamSynchronize(h->stream));
    memcpy(stats, h->hbuf.get(), sizeof(*stats));
    return GS_OK;
}

int gs_slice_reduce_windows(gs_slice_t* h, const void* src, const void* dst, const int64_t* val, uint64_t n,
                            uint64_t window_edges, int op, void* vertices, int64_t* values, uint64_t cap,
                            uint64_t* window_offsets, gs_slice_window_stats* stats, uint64_t cap_windows,
                            uint64_t* n_windows) {
    const char* fn = "gs_slice_reduce_windows";
    GS_TRY(scheck(h, fn));
    if (!n_windows) return fail(GS_ERR_INVALID, "%s: null n_windows", fn);
    if (window_edges == 0) return fail(GS_ERR_INVALID, "%s: window_edges is 0", fn);
    if (!sop_ok(op)) return fail(GS_ERR_INVALID, "%s: unknown op %d", fn, op);
    if (!val && op != GS_SLICE_COUNT) return fail(GS_ERR_INVALID, "%s: without values only GS_SLICE_COUNT applies", fn);
    *n_windows = 0;
    if (n == 0) {
        if (window_offsets) window_offsets[0] = 0;
        h->n = h->ne = h->nv = 0;
        return GS_OK;
    }
    if (!src || !dst) return fail(GS_ERR_INVALID, "%s: null edge buffer", fn);
    const uint64_t nw = (n + window_edges - 1) / window_edges;
    *n_windows = nw;
    if (cap_windows < nw) return fail(GS_ERR_CAPACITY, "%s: %llu windows, capacity %llu", fn, (unsigned long long)nw,
                                      (unsigned long long)cap_windows);
    if (!window_offsets) return fail(GS_ERR_INVALID, "%s: null window_offsets", fn);
    if (cap && (!vertices || !values)) return fail(GS_ERR_INVALID, "%s: null output", fn);
    const uint64_t wmax = std::min(n, window_edges);
    if (wmax > kSliceMaxWindow) return fail(GS_ERR_UNSUPPORTED, "%s: windows of more than 2^30 - 1 edges", fn);
    if (nw > 0xFFFFFFFFull) return fail(GS_ERR_UNSUPPORTED, "%s: more than 2^32 - 1 windows", fn);
    DeviceGuard g(h->device);
    h->n = h->ne = h->nv = 0;
    h->has_val = val != nullptr;
    const bool dev = is_device_pointer(src) && is_device_pointer(dst);
    const bool odev = cap == 0 || (is_device_pointer(vertices) && is_device_pointer(values));
    const size_t isz = h->id_bits / 8;
    // records for host arrays are collected on the device: there are at most as many as entries
    const uint64_t rcap = odev ? cap : std::min<uint64_t>(cap, sentries(h, n));
    GS_TRY(sscratch(h, wmax));
    if (!dev) GS_TRY(h->stage.grow(2 * sup256(wmax * isz), "slice input staging", h->stream));
    if (!odev) GS_TRY(h->ebuf.grow(sup256(rcap * 8) + rcap * 8, "slice records", h->stream));
    GS_TRY(h->woff.grow(nw + 1, "slice window offsets", h->stream));
    GS_TRY(h->dstats.grow(nw, "slice statistics", h->stream));
    const size_t wbytes = (nw + 1) * 8, sbytes = nw * sizeof(gs_slice_window_stats);
    GS_TRY(spinned(h, sizeof(SliceCtl) + wbytes + sbytes));
    void* ov = odev ? vertices : h->ebuf.get();
    long long* ox = odev ? reinterpret_cast<long long*>(values)
                         : reinterpret_cast<long long*>(static_cast<char*>(h->ebuf.get()) + sup256(rcap * 8));
    GS_HIP(hipMemsetAsync(h->ctl.get(), 0, sizeof(SliceCtl), h->stream));
    GS_HIP(hipMemsetAsync(h->woff.get(), 0, 8, h->stream));
    GS_HIP(hipMemsetAsync(h->dstats.get(), 0, sbytes, h->stream));
    if (!odev && rcap) GS_HIP(hipMemsetAsync(h->ebuf.get(), 0, sup256(rcap * 8) + rcap * 8, h->stream));
    uint64_t last = 0;
    for (uint64_t w = 0; w < nw; ++w) {
        const uint64_t off = w * window_edges, m = std::min(window_edges, n - off);
        const uint32_t ne = (uint32_t)sentries(h, m);
        GS_TRY(sbuild(h, src, dst, val, off, (uint32_t)m, dev));
        GS_TRY(sreduce(h, op, ne));
        GS_TRY(sstats(h, ne, h->dstats.get() + w));
        if (h->id_bits == 32)
            hipLaunchKernelGGL(k_slice_append<uint32_t>, dim3(sgrid(ne)), dim3(kSliceThreads), 0, h->stream, (const uint32_t*)h->s.rv,
                               (const long long*)h->s.red, h->ctl.get(), h->woff.get(), (uint32_t)w, static_cast<uint32_t*>(ov), ox, rcap);
        else
            hipLaunchKernelGGL(k_slice_append<int64_t>, dim3(sgrid(ne)), dim3(kSliceThreads), 0, h->stream, (const uint32_t*)h->s.rv,
                               (const long long*)h->s.red, h->ctl.get(), h->woff.get(), (uint32_t)w, static_cast<int64_t*>(ov), ox, rcap);
        GS_HIP(hipGetLastError());
        last = m;
    }
    char* hb = static_cast<char*>(h->hbuf.get());
    GS_HIP(hipMemcpyAsync(hb, h->ctl.get(), sizeof(SliceCtl), hipMemcpyDeviceToHost, h->stream));
    GS_HIP(hipMemcpyAsync(hb + sizeof(SliceCtl), h->woff.get(), wbytes, hipMemcpyDeviceToHost, h->stream));
    GS_HIP(hipMemcpyAsync(hb + sizeof(SliceCtl) + wbytes, h->dstats.get(), sbytes, hipMemcpyDeviceToHost, h->stream));
    if (!odev && rcap) {
        // (the record count is known only after the wait: the whole collection is copied, zero behind the records)
        GS_HIP(hipMemcpyAsync(vertices, ov, rcap * isz, hipMemcpyDeviceToHost, h->stream));
        GS_HIP(hipMemcpyAsync(values, ox, rcap * 8, hipMemcpyDeviceToHost, h->stream));
    }
    GS_HIP(hipStreamSynchronize(h->stream));   // the one host wait of the call
    SliceCtl c;
    memcpy(&c, hb, sizeof(SliceCtl));
    memcpy(window_offsets, hb + sizeof(SliceCtl), wbytes);
    if (stats) memcpy(stats, hb + sizeof(SliceCtl) + wbytes, sbytes);
    if (c.range) return fail(GS_ERR_RANGE, "%s: a vertex id outside [0, %llu); that window and the later ones report nothing", fn,
                             (unsigned long long)h->cap);
    if (c.overflow) return fail(GS_ERR_CAPACITY, "%s: %llu records, capacity %llu", fn, (unsigned long long)window_offsets[nw],
                                (unsigned long long)cap);
    h->n = last;
    h->ne = sentries(h, last);
    h->nv = c.nv;
    return GS_OK;
}

}  // extern "C"
