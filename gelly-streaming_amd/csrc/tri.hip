// tri.hip — per-window exact triangle counts on the device: the reference's WindowTriangles
// (example/WindowTriangles.java:60-65: slice(window, ALL) -> GenerateCandidateEdges (:82-115) ->
// CountTriangles (:118-139) -> timeWindowAll.sum), extern "C" in include/gsgpu.h (gs_tri_*).
//
// The reference emits, per vertex, every pair of larger-id neighbours as a candidate edge and
// counts the candidates that are edges of the window: each triangle once, at its smallest vertex.
// Here a window is counted as set intersections over an oriented adjacency, all on the handle's
// stream, with no host wait inside a window or between windows:
//   1 canonicalise  ids range-checked, self-loops dropped, key = min << bits | max (bits = what the
//                   capacity needs); dropped edges become the all-ones key, which sorts last
//   2 radix sort    hipcub over 2 * bits bits; a key equal to its predecessor is a duplicate. The
//                   number m of simple edges is counted into device memory (Ctl::m) and read
//                   there by every later kernel: the host only knows the window's edge count n.
//   3 orient        low (degree, id) -> high (degree, id) (default), or low id -> high id
//                   (GS_TRI_ORIENT_BY_ID, the reference's rule); key = a << bits | b
//   4 radix sort    again; the first m keys are the out-rows N+(a), each sorted by id. Boundaries
//                   give row start / end per vertex; rows longer than kShortRow go on a list.
//   5 count         triangle (a, b, w) is found once, at its oriented edge a -> b with
//                   w in N+(a) & N+(b) (the orientation is a total order, so acyclic):
//                   k_tri_short: rows of at most kShortRow entries, one oriented edge per lane, the
//                     shorter of the two rows probed into the longer by binary search;
//                   k_tri_long:  one workgroup per longer row a, N+(a) staged in LDS in tiles of
//                     kTile ids (the tile loop runs once for a row that fits); per tile every
//                     b in N+(a) is taken by a 16-lane group whose lanes probe the w in N+(b) into
//                     the tile by binary search. Hits: ballot + popcount per wave, LDS per
//                     workgroup, one 64-bit atomicAdd per workgroup into the window's result slot.
//   6 clear         the per-vertex words the window touched are zeroed again (O(m), not O(capacity))
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <memory>

#include <hipcub/hipcub.hpp>

#include "owned.hpp"

namespace gsgpu {

constexpr uint32_t kShortRow = 64;            // out-rows up to this length: one edge per lane
constexpr uint32_t kTile = 8192;              // ids of N+(a) in LDS at a time (32 KiB)
constexpr uint32_t kTriThreads = 256;
constexpr uint32_t kGroup = 16;               // lanes that share one b in k_tri_long
constexpr unsigned kTriMaxBlocks = 4096;

// control words of one window, in device memory
struct TriCtl {
    uint32_t m;                               // simple edges of the window (after step 2)
    uint32_t n_long;                          // rows on the long list
    uint32_t range;                           // an id outside [0, capacity) was seen (kept for the call)
    uint32_t pad;
};

struct TriArgs {
    TriCtl* ctl;
    uint32_t* deg;                            // [capacity] degree in the simple graph (degree orientation)
    uint32_t* rs;                             // [capacity] start of N+(v) in col
    uint32_t* re;                             // [capacity] its end (rs == re == 0: empty)
    uint32_t bits;                            // id bits in a key
    uint64_t cap;
};

__device__ __forceinline__ uint64_t tri_sentinel(uint32_t bits) {
    return bits == 32 ? ~0ull : ((1ull << (2 * bits)) - 1);
}
__device__ __forceinline__ uint32_t tri_lo(uint64_t k, uint32_t bits) {
    return (uint32_t)(k & (bits == 32 ? 0xFFFFFFFFull : ((1ull << bits) - 1)));
}
__device__ __forceinline__ uint32_t tri_hi(uint64_t k, uint32_t bits) { return (uint32_t)(k >> bits); }

// step 1
template <typename IdT>
__global__ __launch_bounds__(kTriThreads) void k_tri_canon(const IdT* __restrict__ src, const IdT* __restrict__ dst,
                                                           uint32_t n, uint64_t* __restrict__ keys, TriArgs ta) {
    const uint64_t none = tri_sentinel(ta.bits);
    bool bad = false;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const IdT x = src[i], y = dst[i];
        const bool ok = (uint64_t)x < ta.cap && (uint64_t)y < ta.cap;   // (a negative int64 is >= 2^63)
        bad |= !ok;
        const uint32_t u = (uint32_t)x, v = (uint32_t)y;
        keys[i] = (ok && u != v) ? ((uint64_t)(u < v ? u : v) << ta.bits) | (u < v ? v : u) : none;
    }
    if (bad) atomicOr(&ta.ctl->range, 1u);
}

__device__ __forceinline__ bool tri_simple(const uint64_t* __restrict__ k, uint32_t i, uint64_t none) {
    const uint64_t x = k[i];
    return x != none && (i == 0 || x != k[i - 1]);
}

// step 2: m, and the degrees when the orientation needs them
template <bool DEG>
__global__ __launch_bounds__(kTriThreads) void k_tri_mark(const uint64_t* __restrict__ k, uint32_t n, TriArgs ta) {
    const uint64_t none = tri_sentinel(ta.bits);
    const uint32_t lane = threadIdx.x & 63;
    uint32_t c = 0;
    for (uint32_t base = blockIdx.x * blockDim.x; base < n; base += gridDim.x * blockDim.x) {   // (wave-uniform)
        const uint32_t i = base + threadIdx.x;
        const bool ok = i < n && tri_simple(k, i, none);
        c += ok;
        if (DEG) {
            // the keys are sorted by their smaller id: a wave adds each run of equal smaller ids
            // once, from the run's first lane (repeated edges sit inside the run they repeat)
            const uint32_t a = (i < n && k[i] != none) ? tri_hi(k[i], ta.bits) : kInvalid;
            const uint32_t before = __shfl_up(a, 1, 64);
            const unsigned long long heads = __ballot(lane == 0 || a != before);
            const unsigned long long valid = __ballot(ok);
            if ((heads >> lane) & 1ull) {
                const unsigned long long above = lane == 63 ? 0ull : (heads >> (lane + 1)) << (lane + 1);
                const unsigned long long upto = above ? ((above & (~above + 1)) - 1) : ~0ull;   // lanes below the next head
                const uint32_t cnt = __popcll(valid & upto & (~0ull << lane));
                if (cnt) atomicAdd(&ta.deg[a], cnt);
            }
            if (ok) atomicAdd(&ta.deg[tri_lo(k[i], ta.bits)], 1u);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&ta.ctl->m, c);
}

// step 3
template <bool DEG>
__global__ __launch_bounds__(kTriThreads) void k_tri_orient(const uint64_t* __restrict__ k, uint32_t n,
                                                            uint64_t* __restrict__ out, TriArgs ta) {
    const uint64_t none = tri_sentinel(ta.bits);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        uint64_t o = none;
        if (tri_simple(k, i, none)) {
            uint32_t a = tri_hi(k[i], ta.bits), b = tri_lo(k[i], ta.bits);      // a < b
            if (DEG && ta.deg[a] > ta.deg[b]) { const uint32_t t = a; a = b; b = t; }
            o = ((uint64_t)a << ta.bits) | b;
        }
        out[i] = o;
    }
}

// step 4: the first m sorted keys are the rows; col = their b; row bounds per a
__global__ __launch_bounds__(kTriThreads) void k_tri_rows(const uint64_t* __restrict__ k, uint32_t* __restrict__ col,
                                                          TriArgs ta) {
    const uint32_t m = ta.ctl->m;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        const uint32_t a = tri_hi(k[i], ta.bits);
        col[i] = tri_lo(k[i], ta.bits);
        if (i == 0 || tri_hi(k[i - 1], ta.bits) != a) ta.rs[a] = i;
        if (i + 1 == m || tri_hi(k[i + 1], ta.bits) != a) ta.re[a] = i + 1;
    }
}

// rows longer than kShortRow, in any order (at most m / (kShortRow + 1) of them)
__global__ __launch_bounds__(kTriThreads) void k_tri_bins(const uint64_t* __restrict__ k, uint32_t* __restrict__ long_rows,
                                                          TriArgs ta) {
    const uint32_t m = ta.ctl->m;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        const uint32_t a = tri_hi(k[i], ta.bits);
        if (i != 0 && tri_hi(k[i - 1], ta.bits) == a) continue;
        if (ta.re[a] - i > kShortRow) long_rows[atomicAdd(&ta.ctl->n_long, 1u)] = a;
    }
}

// is x among the n ascending ids at p (global memory or LDS)
__device__ __forceinline__ bool tri_has(const uint32_t* p, uint32_t n, uint32_t x) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (p[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo < n && p[lo] == x;
}

// a workgroup's hits: one 64-bit atomicAdd into the window's slot
__device__ __forceinline__ void tri_flush(unsigned long long c, unsigned long long* __restrict__ result) {
    __shared__ unsigned long long part[kTriThreads / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (uint32_t w = 0; w < kTriThreads / 64; ++w) s += part[w];
        if (s) atomicAdd(result, s);
    }
}

// step 5, short rows: one oriented edge a -> b per lane
template <bool LOCAL>
__global__ __launch_bounds__(kTriThreads) void k_tri_short(const uint64_t* __restrict__ k, const uint32_t* __restrict__ col,
                                                           TriArgs ta, unsigned long long* __restrict__ result,
                                                           unsigned long long* __restrict__ local) {
    const uint32_t m = ta.ctl->m;
    unsigned long long c = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        const uint32_t a = tri_hi(k[i], ta.bits), b = col[i];
        const uint32_t as = ta.rs[a], al = ta.re[a] - as;
        if (al > kShortRow) continue;                         // k_tri_long's
        const uint32_t bs = ta.rs[b], bl = ta.re[b] - bs;
        if (bl == 0 || al < 2) continue;
        const bool swap = bl < al;                            // walk the shorter row, probe the longer
        const uint32_t* walk = col + (swap ? bs : as);
        const uint32_t* probe = col + (swap ? as : bs);
        const uint32_t wl = swap ? bl : al, pl = swap ? al : bl;
        uint32_t hits = 0;
        for (uint32_t j = 0; j < wl; ++j) {
            const uint32_t w = walk[j];
            if (tri_has(probe, pl, w)) {
                ++hits;
                if (LOCAL) atomicAdd(&local[w], 1ull);
            }
        }
        if (LOCAL && hits) {
            atomicAdd(&local[a], (unsigned long long)hits);
            atomicAdd(&local[b], (unsigned long long)hits);
        }
        c += hits;
    }
    tri_flush(c, result);
}

// step 5, long rows: one workgroup per row a
template <bool LOCAL>
__global__ __launch_bounds__(kTriThreads) void k_tri_long(const uint32_t* __restrict__ long_rows,
                                                          const uint32_t* __restrict__ col, TriArgs ta,
                                                          unsigned long long* __restrict__ result,
                                                          unsigned long long* __restrict__ local) {
    __shared__ uint32_t tile[kTile];
    __shared__ unsigned long long row_hits;                   // LOCAL: hits of the current row a
    constexpr uint32_t kGroups = kTriThreads / kGroup;
    const uint32_t g = threadIdx.x / kGroup, gl = threadIdx.x % kGroup;
    const uint32_t gshift = ((threadIdx.x & 63) / kGroup) * kGroup;   // the group's lanes within its wave's ballot
    const uint32_t n_long = ta.ctl->n_long;
    unsigned long long wave_hits = 0;                         // wave-uniform
    for (uint32_t r = blockIdx.x; r < n_long; r += gridDim.x) {
        const uint32_t a = long_rows[r];
        const uint32_t as = ta.rs[a], al = ta.re[a] - as;
        unsigned long long wave_row = 0;
        if (LOCAL && threadIdx.x == 0) row_hits = 0;
        for (uint32_t t0 = 0; t0 < al; t0 += kTile) {
            const uint32_t tl = min(kTile, al - t0);
            __syncthreads();                                  // the last tile's probes are done
            for (uint32_t i = threadIdx.x; i < tl; i += kTriThreads) tile[i] = col[as + t0 + i];
            __syncthreads();
            const uint32_t tmin = tile[0], tmax = tile[tl - 1];
            for (uint32_t b0 = 0; b0 < al; b0 += kGroups) {   // (workgroup-uniform trip count)
                const uint32_t bi = b0 + g;
                uint32_t b = 0, bs = 0, bl = 0;
                if (bi < al) {
                    b = col[as + bi];
                    bs = ta.rs[b];
                    bl = ta.re[b] - bs;
                }
                uint32_t ghits = 0;
                for (uint32_t j = gl; __any(j < bl); j += kGroup) {   // (wave-uniform trip count)
                    bool hit = false;
                    uint32_t w = 0;
                    if (j < bl) {
                        w = col[bs + j];
                        hit = w >= tmin && w <= tmax && tri_has(tile, tl, w);
                    }
                    const unsigned long long mask = __ballot(hit);
                    wave_row += __popcll(mask);
                    if (LOCAL) {
                        ghits += __popcll((mask >> gshift) & ((1ull << kGroup) - 1));
                        if (hit) atomicAdd(&local[w], 1ull);
                    }
                }
                if (LOCAL && gl == 0 && ghits) atomicAdd(&local[b], (unsigned long long)ghits);
            }
        }
        wave_hits += wave_row;
        if (LOCAL) {
            if ((threadIdx.x & 63) == 0 && wave_row) atomicAdd(&row_hits, wave_row);
            __syncthreads();
            if (threadIdx.x == 0 && row_hits) atomicAdd(&local[a], row_hits);
            __syncthreads();                                  // (row_hits is reset for the next row)
        }
    }
    tri_flush((threadIdx.x & 63) == 0 ? wave_hits : 0ull, result);
}

// step 6: the per-vertex words of the window's vertices back to zero
__global__ __launch_bounds__(kTriThreads) void k_tri_clear(const uint64_t* __restrict__ k, TriArgs ta, int deg) {
    const uint32_t m = ta.ctl->m;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        const uint32_t a = tri_hi(k[i], ta.bits), b = tri_lo(k[i], ta.bits);
        ta.rs[a] = 0;
        ta.re[a] = 0;
        if (deg) {
            ta.deg[a] = 0;
            ta.deg[b] = 0;
        }
    }
}

}  // namespace gsgpu

using namespace gsgpu;

struct gs_tri {
    uint64_t cap = 0;
    uint32_t id_bits = 64, bits = 1, flags = 0;
    int device = 0;
    Stream own;
    hipStream_t stream = nullptr;              // own, or the caller's (gs_tri_set_stream)
    DevBuf<uint32_t> vtx;                      // deg | rs | re, capacity words each, zero between windows
    DevBuf<TriCtl> ctl;
    DevBuf<unsigned long long> results;        // one slot per window of a call
    Pinned<unsigned long long> hres;           // pinned mirror of results, then of ctl
    size_t hres_cap = 0;
    DevBuf<> tmp;                              // keys x 2, col, long rows, sort temporaries: by the largest window seen
    DevBuf<> stage;                            // host inputs of one window
    DevBuf<unsigned long long> local;          // per-vertex counts when the caller's array is on the host
};

namespace {

constexpr uint64_t kTriMaxCap = 1ull << 32;
constexpr uint64_t kTriMaxWindow = 0x7FFFFFFFull;     // hipcub's item count is an int

int tcheck(gs_tri_t* h, const char* fn) { return h ? GS_OK : fail(GS_ERR_INVALID, "%s: null handle", fn); }

unsigned tgrid(uint64_t items) {
    const uint64_t b = (items + kTriThreads - 1) / kTriThreads;
    return (unsigned)std::min<uint64_t>(std::max<uint64_t>(b, 1), kTriMaxBlocks);
}

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// the scratch layout for windows of up to n edges
struct TriScratch {
    uint64_t *ka = nullptr, *kb = nullptr;
    uint32_t *col = nullptr, *long_rows = nullptr;
    void* sort = nullptr;
    size_t sort_bytes = 0;
};

int tscratch(gs_tri_t* h, uint64_t n, TriScratch& s) {
    GS_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, s.sort_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)n,
                                              0, (int)(2 * h->bits), h->stream));
    const size_t kbytes = up256(n * 8), cbytes = up256(n * 4), lbytes = up256((n / (kShortRow + 1) + 1) * 4);
    GS_TRY(h->tmp.grow(2 * kbytes + cbytes + lbytes + up256(s.sort_bytes), "triangle scratch", h->stream));
    char* p = static_cast<char*>(h->tmp.get());
    s.ka = reinterpret_cast<uint64_t*>(p);
    s.kb = reinterpret_cast<uint64_t*>(p + kbytes);
    s.col = reinterpret_cast<uint32_t*>(p + 2 * kbytes);
    s.long_rows = reinterpret_cast<uint32_t*>(p + 2 * kbytes + cbytes);
    s.sort = p + 2 * kbytes + cbytes + lbytes;
    return GS_OK;
}

// one window of n device edges, counted into *result (and local, when not null); enqueues only
template <bool LOCAL>
int twindow(gs_tri_t* h, const TriScratch& s, const void* src, const void* dst, uint32_t n,
            unsigned long long* result, unsigned long long* local) {
    const bool deg = !(h->flags & GS_TRI_ORIENT_BY_ID);
    const size_t cap = (size_t)h->cap;
    uint32_t* v = h->vtx.get();
    const TriArgs ta{h->ctl.get(), v, v + cap, v + 2 * cap, h->bits, h->cap};
    const dim3 grid(tgrid(n)), block(kTriThreads);
    const int end_bit = (int)(2 * h->bits);
    size_t sort_bytes = s.sort_bytes;
    GS_HIP(hipMemsetAsync(h->ctl.get(), 0, offsetof(TriCtl, range), h->stream));      // m, n_long
    if (h->id_bits == 32)
        hipLaunchKernelGGL(k_tri_canon<uint32_t>, grid, block, 0, h->stream, (const uint32_t*)src, (const uint32_t*)dst, n, s.ka, ta);
    else
        hipLaunchKernelGGL(k_tri_canon<int64_t>, grid, block, 0, h->stream, (const int64_t*)src, (const int64_t*)dst, n, s.ka, ta);
    GS_HIP(hipGetLastError());
    GS_HIP(hipcub::DeviceRadixSort::SortKeys(s.sort, sort_bytes, (const uint64_t*)s.ka, s.kb, (int)n, 0, end_bit, h->stream));
    if (deg) {
        hipLaunchKernelGGL(k_tri_mark<true>, grid, block, 0, h->stream, (const uint64_t*)s.kb, n, ta);
        hipLaunchKernelGGL(k_tri_orient<true>, grid, block, 0, h->stream, (const uint64_t*)s.kb, n, s.ka, ta);
    } else {
        hipLaunchKernelGGL(k_tri_mark<false>, grid, block, 0, h->stream, (const uint64_t*)s.kb, n, ta);
        hipLaunchKernelGGL(k_tri_orient<false>, grid, block, 0, h->stream, (const uint64_t*)s.kb, n, s.ka, ta);
    }
    GS_HIP(hipGetLastError());
    GS_HIP(hipcub::DeviceRadixSort::SortKeys(s.sort, sort_bytes, (const uint64_t*)s.ka, s.kb, (int)n, 0, end_bit, h->stream));
    hipLaunchKernelGGL(k_tri_rows, grid, block, 0, h->stream, (const uint64_t*)s.kb, s.col, ta);
    hipLaunchKernelGGL(k_tri_bins, grid, block, 0, h->stream, (const uint64_t*)s.kb, s.long_rows, ta);
    hipLaunchKernelGGL(k_tri_short<LOCAL>, grid, block, 0, h->stream, (const uint64_t*)s.kb, (const uint32_t*)s.col, ta,
                       result, local);
    const dim3 lgrid((unsigned)std::min<uint64_t>(n / (kShortRow + 1) + 1, kTriMaxBlocks));
    hipLaunchKernelGGL(k_tri_long<LOCAL>, lgrid, block, 0, h->stream, (const uint32_t*)s.long_rows, (const uint32_t*)s.col,
                       ta, result, local);
    hipLaunchKernelGGL(k_tri_clear, grid, block, 0, h->stream, (const uint64_t*)s.kb, ta, deg ? 1 : 0);
    GS_HIP(hipGetLastError());
    return GS_OK;
}

// the window's edges where the kernels can read them
int tinput(gs_tri_t* h, const void* src, const void* dst, uint64_t off, uint64_t n, bool dev, const void*& a, const void*& b) {
    const size_t esz = h->id_bits / 8;
    if (dev) {
        a = static_cast<const char*>(src) + off * esz;
        b = static_cast<const char*>(dst) + off * esz;
        return GS_OK;
    }
    char* s0 = static_cast<char*>(h->stage.get());
    char* s1 = s0 + up256(n * esz);
    GS_HIP(hipMemcpyAsync(s0, static_cast<const char*>(src) + off * esz, n * esz, hipMemcpyDefault, h->stream));
    GS_HIP(hipMemcpyAsync(s1, static_cast<const char*>(dst) + off * esz, n * esz, hipMemcpyDefault, h->stream));
    a = s0;
    b = s1;
    return GS_OK;
}

// results[0 .. nres) and the control words to the host; the one host wait of a call
int tfinish(gs_tri_t* h, uint64_t nres, TriCtl& c) {
    const size_t words = nres + 2;
    if (h->hres_cap < words) {
        GS_TRY(h->hres.alloc(words, "triangle results"));
        h->hres_cap = words;
    }
    GS_HIP(hipMemcpyAsync(h->hres.get(), h->results.get(), nres * 8, hipMemcpyDeviceToHost, h->stream));
    GS_HIP(hipMemcpyAsync(h->hres.get() + nres, h->ctl.get(), sizeof(TriCtl), hipMemcpyDeviceToHost, h->stream));
    GS_HIP(hipStreamSynchronize(h->stream));
    memcpy(&c, h->hres.get() + nres, sizeof(TriCtl));
    if (c.range) return fail(GS_ERR_RANGE, "a vertex id outside [0, %llu); no count is reported", (unsigned long long)h->cap);
    return GS_OK;
}

}  // namespace

extern "C" {

int gs_tri_create(gs_tri_t** out, uint64_t vertex_capacity, uint32_t id_bits, int device, uint32_t flags) {
    if (!out) return fail(GS_ERR_INVALID, "gs_tri_create: null out");
    *out = nullptr;
    if (flags & ~(uint32_t)GS_TRI_ORIENT_BY_ID) return fail(GS_ERR_INVALID, "gs_tri_create: unknown flags 0x%x", flags);
    if (id_bits != 32 && id_bits != 64) return fail(GS_ERR_INVALID, "gs_tri_create: id_bits must be 32 or 64");
    if (vertex_capacity == 0 || vertex_capacity > kTriMaxCap)
        return fail(GS_ERR_INVALID, "gs_tri_create: vertex_capacity must be in [1, 2^32]");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return fail(GS_ERR_HIP, "gs_tri_create: no HIP device available");
    }
    if (device < 0 || device >= ndev) return fail(GS_ERR_INVALID, "gs_tri_create: device %d of %d", device, ndev);
    DeviceGuard g(device);
    gs_tri_t* h = new gs_tri_t();
    struct Destroy { void operator()(gs_tri_t* p) const { (void)gs_tri_destroy(p); } };
    std::unique_ptr<gs_tri_t, Destroy> guard(h);      // a failure below destroys what exists so far
    h->cap = vertex_capacity;
    h->id_bits = id_bits;
    h->flags = flags;
    h->device = device;
    while (h->bits < 32 && (1ull << h->bits) < vertex_capacity) ++h->bits;
    GS_TRY(h->own.create());
    h->stream = h->own;
    GS_TRY(h->vtx.grow((size_t)vertex_capacity * 3, "gs_tri_create: per-vertex rows"));
    GS_TRY(h->ctl.grow(1, "gs_tri_create: control words"));
    GS_HIP(hipMemsetAsync(h->vtx.get(), 0, (size_t)vertex_capacity * 3 * sizeof(uint32_t), h->stream));
    GS_HIP(hipMemsetAsync(h->ctl.get(), 0, sizeof(TriCtl), h->stream));
    GS_HIP(hipStreamSynchronize(h->stream));
    *out = guard.release();
    return GS_OK;
}

int gs_tri_destroy(gs_tri_t* h) {
    if (!h) return GS_OK;
    DeviceGuard g(h->device);
    if (h->own) (void)hipStreamSynchronize(h->own);
    if (h->stream && h->stream != h->own.get()) (void)hipStreamSynchronize(h->stream);
    delete h;                                  // the owners free what it holds (owned.hpp)
    return GS_OK;
}

int gs_tri_set_stream(gs_tri_t* h, void* s) {
    GS_TRY(tcheck(h, "gs_tri_set_stream"));
    h->stream = static_cast<hipStream_t>(s);
    return GS_OK;
}

int gs_tri_get_stream(gs_tri_t* h, void** s) {
    GS_TRY(tcheck(h, "gs_tri_get_stream"));
    if (!s) return fail(GS_ERR_INVALID, "gs_tri_get_stream: null out");
    *s = h->stream;
    return GS_OK;
}

int gs_tri_sync(gs_tri_t* h) {
    GS_TRY(tcheck(h, "gs_tri_sync"));
    DeviceGuard g(h->device);
    GS_HIP(hipStreamSynchronize(h->stream));
    return GS_OK;
}

int gs_tri_count_windows(gs_tri_t* h, const void* src, const void* dst, uint64_t n, uint64_t window_edges,
                         uint64_t* counts, uint64_t cap, uint64_t* n_windows) {
    GS_TRY(tcheck(h, "gs_tri_count_windows"));
    if (!n_windows) return fail(GS_ERR_INVALID, "gs_tri_count_windows: null n_windows");
    if (window_edges == 0) return fail(GS_ERR_INVALID, "gs_tri_count_windows: window_edges is 0");
    *n_windows = 0;
    if (n == 0) return GS_OK;
    if (!src || !dst) return fail(GS_ERR_INVALID, "gs_tri_count_windows: null edge buffer");
    const uint64_t nw = (n + window_edges - 1) / window_edges;
    *n_windows = nw;
    if (cap < nw) return fail(GS_ERR_CAPACITY, "gs_tri_count_windows: %llu windows, capacity %llu",
                              (unsigned long long)nw, (unsigned long long)cap);
    if (!counts) return fail(GS_ERR_INVALID, "gs_tri_count_windows: null counts");
    const uint64_t wmax = std::min(n, window_edges);
    if (wmax > kTriMaxWindow) return fail(GS_ERR_UNSUPPORTED, "gs_tri_count_windows: windows of more than 2^31 - 1 edges");
    DeviceGuard g(h->device);
    const bool dev = is_device_pointer(src) && is_device_pointer(dst);
    TriScratch s;
    GS_TRY(tscratch(h, wmax, s));
    if (!dev) GS_TRY(h->stage.grow(2 * up256(wmax * (h->id_bits / 8)), "triangle input staging", h->stream));
    GS_TRY(h->results.grow(nw, "triangle results", h->stream));
    GS_HIP(hipMemsetAsync(h->results.get(), 0, nw * 8, h->stream));
    GS_HIP(hipMemsetAsync(h->ctl.get(), 0, sizeof(TriCtl), h->stream));
    for (uint64_t w = 0; w < nw; ++w) {
        const uint64_t off = w * window_edges, m = std::min(window_edges, n - off);
        const void *a, *b;
        GS_TRY(tinput(h, src, dst, off, m, dev, a, b));
        GS_TRY(twindow<false>(h, s, a, b, (uint32_t)m, h->results.get() + w, nullptr));
    }
    TriCtl c;
    GS_TRY(tfinish(h, nw, c));
    for (uint64_t w = 0; w < nw; ++w) counts[w] = h->hres.get()[w];
    return GS_OK;
}

int gs_tri_count_local(gs_tri_t* h, const void* src, const void* dst, uint64_t n,
                       uint64_t* local, uint64_t* triangles, uint64_t* simple_edges) {
    GS_TRY(tcheck(h, "gs_tri_count_local"));
    if (!triangles) return fail(GS_ERR_INVALID, "gs_tri_count_local: null triangles");
    if (n && (!src || !dst)) return fail(GS_ERR_INVALID, "gs_tri_count_local: null edge buffer");
    if (n > kTriMaxWindow) return fail(GS_ERR_UNSUPPORTED, "gs_tri_count_local: more than 2^31 - 1 edges");
    DeviceGuard g(h->device);
    const bool ldev = local && is_device_pointer(local);
    unsigned long long* dl = nullptr;
    if (local) {
        if (!ldev) GS_TRY(h->local.grow((size_t)h->cap, "per-vertex triangle counts", h->stream));
        dl = ldev ? reinterpret_cast<unsigned long long*>(local) : h->local.get();
    }
    TriCtl c{};
    uint64_t total = 0;
    if (n) {
        const bool dev = is_device_pointer(src) && is_device_pointer(dst);
        TriScratch s;
        GS_TRY(tscratch(h, n, s));
        if (!dev) GS_TRY(h->stage.grow(2 * up256(n * (h->id_bits / 8)), "triangle input staging", h->stream));
        GS_TRY(h->results.grow(1, "triangle results", h->stream));
        GS_HIP(hipMemsetAsync(h->results.get(), 0, 8, h->stream));
        GS_HIP(hipMemsetAsync(h->ctl.get(), 0, sizeof(TriCtl), h->stream));
        if (dl) GS_HIP(hipMemsetAsync(dl, 0, (size_t)h->cap * 8, h->stream));
        const void *a, *b;
        GS_TRY(tinput(h, src, dst, 0, n, dev, a, b));
        if (dl) GS_TRY(twindow<true>(h, s, a, b, (uint32_t)n, h->results.get(), dl));
        else GS_TRY(twindow<false>(h, s, a, b, (uint32_t)n, h->results.get(), nullptr));
        GS_TRY(tfinish(h, 1, c));
        total = h->hres.get()[0];
    } else if (dl) {
        GS_HIP(hipMemsetAsync(dl, 0, (size_t)h->cap * 8, h->stream));
    }
    if (local && !ldev) GS_HIP(hipMemcpyAsync(local, dl, (size_t)h->cap * 8, hipMemcpyDeviceToHost, h->stream));
    if (local) GS_HIP(hipStreamSynchronize(h->stream));
    *triangles = total;
    if (simple_edges) *simple_edges = c.m;
    return GS_OK;
}

}  // extern "C"
