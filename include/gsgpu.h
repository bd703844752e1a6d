/*
 * gsgpu.h — C ABI of libgsgpu.so: MI355X (gfx950) streaming Connected Components for the
 * Gelly Streaming `ConnectedComponents` SummaryBulkAggregation hot path.
 *
 * Reference interfaces replaced (paths relative to the reference's
 * src/main/java/org/apache/flink/graph/streaming/):
 *
 *   gs_cc_create / gs_cc_reset   new DisjointSet<K>() as the fold's initial value
 *                                (library/ConnectedComponents.java:52-54, summaries/DisjointSet.java:31-34)
 *   gs_cc_fold / gs_cc_fold_pairs  EdgesFold.foldEdges -> UpdateCC: ds.union(u, v) per edge
 *                                (EdgesFold.java:47, library/ConnectedComponents.java:83-85,
 *                                 summaries/DisjointSet.java:92-118, SummaryBulkAggregation.java:121-123)
 *   gs_cc_merge                  DisjointSet.merge(other)  (summaries/DisjointSet.java:127-131)
 *   gs_cc_combine                CombineCC.reduce(s1, s2): merge the smaller summary into the larger
 *                                (library/ConnectedComponents.java:116-125)
 *   gs_cc_close_window           the Merger step that emits the cumulative summary per window
 *                                (SummaryAggregation.java:106-119; transientState=false)
 *   gs_cc_find                   DisjointSet.find (summaries/DisjointSet.java:66-80; -1 = null)
 *   gs_cc_stats                  getMatches().size() and the number of components
 *                                (summaries/DisjointSet.java:44-46)
 *   gs_cc_emit_dense / _pairs    the emitted summary as canonical (vertex, min-id) labels:
 *                                what getMatches()+find() give FlattenSet
 *                                (example/ConnectedComponentsExample.java:143-156) and toString
 *                                groups by (summaries/DisjointSet.java:133-150), canonicalised
 *   gs_cc_export_marks           the partial summary that crosses the windowAll / tree exchange
 *                                (SummaryBulkAggregation.java:81, SummaryTreeReduce.java:95-123)
 *
 * Conventions: every function returns 0 (GS_OK) or a negative GS_ERR_* code; the message of the
 * last failure on the calling thread is gs_last_error(). No C++ exception crosses the ABI.
 * Buffers passed in may be host (pageable or pinned) or device pointers; the caller keeps
 * ownership of them, the library owns all device state of a handle. Input buffers of a fold must
 * stay unchanged until the handle's stream has run it (gs_cc_sync): host edges are copied
 * asynchronously (double-buffered staging, gs_cc_config.staging_edges per chunk). One handle per subtask
 * thread; calls on one handle must be serialised by the caller; different handles may be used
 * concurrently. All work of a handle is ordered on its HIP stream (gs_cc_set_stream).
 */
#ifndef GSGPU_H
#define GSGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSGPU_VERSION 2

enum {
    GS_OK = 0,
    GS_ERR_INVALID = -1,      /* bad argument                                           */
    GS_ERR_HIP = -2,          /* HIP runtime failure                                    */
    GS_ERR_RANGE = -3,        /* a vertex id outside [0, vertex_capacity)               */
    GS_ERR_NOMEM = -4,        /* device allocation failed                               */
    GS_ERR_STATE = -5,        /* call not valid in the handle's current state           */
    GS_ERR_UNSUPPORTED = -6,  /* feature not built / not enabled on this handle         */
    GS_ERR_CAPACITY = -7,     /* output buffer too small                                */
    GS_ERR_COMM = -8          /* collective / communicator failure (RCCL)               */
};

/* gs_cc_config.flags */
enum {
    GS_CC_TRACK_MARKS = 1u << 0, /* keep per-vertex marks of this window's hooks, needed by
                                    gs_cc_export_marks (multi-GPU / multi-handle merge)    */
    GS_CC_SPARSE_IDS = 1u << 1   /* id_bits 64 only: ids are ANY 64-bit values (Java long,
                                    negatives included), hashed to slots on the device;
                                    vertex_capacity = most distinct ids (<= 2^30). Canonical
                                    labels are still the minimum id of each component.
                                    gs_cc_emit_dense, gs_cc_emit_delta and
                                    gs_cc_labels_device are not available in this mode; with
                                    GS_CC_TRACK_MARKS the exchange carries int64 pairs.      */
};

typedef struct gs_cc gs_cc_t;

typedef struct gs_cc_config {
    uint32_t struct_size;       /* sizeof(gs_cc_config)                                    */
    uint32_t id_bits;           /* 32 (int/uint32 ids) or 64 (long ids, the reference's K=Long) */
    uint64_t vertex_capacity;   /* ids must lie in [0, vertex_capacity); <= 2^32 - 1
                                   (GS_CC_SPARSE_IDS: the number of distinct ids, <= 2^30)   */
    int32_t  device;            /* HIP device ordinal                                      */
    uint32_t flags;             /* GS_CC_*                                                 */
    uint64_t staging_edges;     /* staging chunk of host-pointer folds, 2 slots (0 = 2^24) */
} gs_cc_config;

/* ---- lifetime ---- */
int gs_cc_create(gs_cc_t** out, const gs_cc_config* cfg);
int gs_cc_destroy(gs_cc_t* h);
int gs_cc_reset(gs_cc_t* h);                        /* back to an empty DisjointSet          */
/* Orders all later work of the handle on hip_stream (NULL = the HIP null stream). A new handle
 * runs on a non-blocking stream of its own; set the caller's stream before folding device buffers
 * the caller produced on it. */
int gs_cc_set_stream(gs_cc_t* h, void* hip_stream);
int gs_cc_get_stream(gs_cc_t* h, void** hip_stream);
int gs_cc_sync(gs_cc_t* h);                         /* wait for the handle's stream; reports
                                                       deferred device errors (GS_ERR_RANGE) */

/* ---- UpdateCC / DisjointSet.union over a batch ----
 * src/dst: n ids each (id_bits wide). pairs: n interleaved (src, dst) ids. Duplicates and
 * self-loops are allowed: union(u,u) makes u a singleton (DisjointSet.java:94-105). */
int gs_cc_fold(gs_cc_t* h, const void* src, const void* dst, uint64_t n);
int gs_cc_fold_pairs(gs_cc_t* h, const void* pairs, uint64_t n);

/* ---- DisjointSet.merge / CombineCC ---- (both handles on one device) */
int gs_cc_merge(gs_cc_t* into, gs_cc_t* from);
/* CombineCC.reduce(s1, s2): if |s1| <= |s2| then s2.merge(s1), *result = s2; else s1.merge(s2),
 * *result = s1 (sizes = getMatches().size()). */
int gs_cc_combine(gs_cc_t* s1, gs_cc_t* s2, gs_cc_t** result);

/* ---- Merger / emission ----
 * close_window fully compresses the summary: afterwards every seen vertex's label is the
 * minimum vertex id of its component, resident on the device (gs_cc_labels_device). */
int gs_cc_close_window(gs_cc_t* h);
int gs_cc_stats(gs_cc_t* h, uint64_t* n_vertices, uint64_t* n_components);
/* labels[v] for v < n: canonical label of v, or -1 if v is not in the summary.
 * Output element width = id_bits. Implies close_window. */
int gs_cc_emit_dense(gs_cc_t* h, void* labels, uint64_t n);
/* (vertex, label) pairs of every vertex in the summary, sorted by vertex.
 * Writes min(cap, |V|) pairs, *n_out = |V|; GS_ERR_CAPACITY if cap < |V|. Implies close_window. */
int gs_cc_emit_pairs(gs_cc_t* h, void* vertices, void* labels, uint64_t cap, uint64_t* n_out);
/* Per-window DELTA of the emission (what a host-side Merger / FlattenSet consumer needs to keep its
 * copy of the cumulative summary, SummaryAggregation.java:110-111, ConnectedComponentsExample.java:
 * 143-156, at O(changes) PCIe cost): the (vertex, label) pairs, sorted by vertex, of every vertex
 * that is new or whose canonical label changed since the previous gs_cc_emit_delta call (the first
 * call, and the first after gs_cc_reset, returns the whole emission). Writes the pairs if they fit:
 * *n_out = their number; if cap < *n_out, GS_ERR_CAPACITY and NOTHING is consumed (call again with
 * a bigger buffer). Applying every delta in order to a map reproduces gs_cc_emit_pairs. Output
 * element width = id_bits; vertices/labels host or device. Dense ids only. Implies close_window. */
int gs_cc_emit_delta(gs_cc_t* h, void* vertices, void* labels, uint64_t cap, uint64_t* n_out);
/* gs_cc_emit_delta, enqueued only (the per-window Merger emission without a host wait): the delta is
 * computed on the handle's stream into one of two device slots — the next fold can be enqueued at
 * once — and its size into a pinned word. gs_cc_emit_wait copies it to vertices/labels (device or
 * host memory; pinned host memory copies at full PCIe rate) while the GPU runs whatever was enqueued
 * after it; the buffers and *n_out are valid once gs_cc_emit_wait has returned that emission. An
 * emission that did not fit cap consumed nothing (*n_out = its size, gs_cc_emit_wait returns
 * GS_ERR_CAPACITY) and its pairs stay in the next delta. At most two emissions pending per handle;
 * gs_cc_emit_delta waits for pending ones first. */
int gs_cc_emit_delta_async(gs_cc_t* h, void* vertices, void* labels, uint64_t cap, uint64_t* n_out);
/* Waits for async delta emissions, oldest first, until at most `keep` are pending (0: all; also done
 * by gs_cc_sync), writing their *n_out. GS_ERR_CAPACITY if one of them did not fit its cap. */
int gs_cc_emit_wait(gs_cc_t* h, uint32_t keep);
/* Order-independent checksum of the canonical emission (definition shared with oracle/:
 * sum over seen v of splitmix64(v ^ splitmix64(label ^ 0xD1B54A32D192ED03))). Implies close_window. */
int gs_cc_checksum(gs_cc_t* h, uint64_t* checksum, uint64_t* n_vertices, uint64_t* n_components);
/* DisjointSet.find for n ids: roots[i] = current root of ids[i], -1 if unknown (null).
 * The root is the canonical label (roots are always component minima). */
int gs_cc_find(gs_cc_t* h, const void* ids, void* roots, uint64_t n);
/* as gs_cc_find, and found[i] = 1 if ids[i] is in the summary, 0 if not (null) — needed where -1
 * is itself a valid id (GS_CC_SPARSE_IDS). found may be NULL. Implies close_window. */
int gs_cc_find_flags(gs_cc_t* h, const void* ids, void* roots, uint8_t* found, uint64_t n);
/* device pointer to the uint32 label/parent array (length vertex_capacity, 0xFFFFFFFF = unseen). */
int gs_cc_labels_device(gs_cc_t* h, const void** dev_ptr);

/* ---- partial-summary exchange (windowAll / tree merge) ----
 * Requires GS_CC_TRACK_MARKS. Writes the (vertex, root) pairs (uint32, interleaved; with
 * GS_CC_SPARSE_IDS (id, id of the root's component) as int64, interleaved, 16 B per pair) of
 * every vertex whose root status changed in this handle since the last export (roots it hooked,
 * singletons made by self-loops: the handle's hook log, at most 2 x vertex_capacity entries), and
 * consumes them; pairs past cap stay for the next export. Folding these pairs into another
 * summary (gs_cc_fold_pairs, 32-bit ids regardless of id_bits via gs_cc_fold_pairs32) transfers
 * all connectivity this handle gained. */
int gs_cc_export_marks(gs_cc_t* h, void* pairs, uint64_t cap, uint64_t* n_out);
int gs_cc_fold_pairs32(gs_cc_t* h, const void* pairs, uint64_t n);
/* as gs_cc_export_marks, but only enqueued on the handle's stream: the pair count lands in the
 * device uint64 *dev_count (no host synchronisation; a collective can take it from there).
 * pairs and dev_count are device pointers; cap must be >= 2 x vertex_capacity (never overflows). */
int gs_cc_export_marks_async(gs_cc_t* h, void* pairs, uint64_t cap, void* dev_count);
/* The giant pre-filter alone (UpdateCC's read-only half; what a GS_MERGE_PREFILTER sender runs):
 * the edges (src[i], dst[i]), i < n (id_bits wide, host or device), that survive this handle's
 * giant filter — NOT both endpoints in the giant component it last picked — written as uint32
 * (u, v) pairs to the device buffer pairs (cap >= n pairs); *n_out = their number (synchronous).
 * Nothing is folded. Dense ids only. Out-of-range ids are skipped and reported (GS_ERR_RANGE). */
int gs_cc_filter_edges(gs_cc_t* h, const void* src, const void* dst, uint64_t n, void* pairs, uint64_t cap,
                       uint64_t* n_out);
/* Pause (on = 0) / resume (on = 1) marking on a GS_CC_TRACK_MARKS handle: folds while paused leave
 * no marks (a replica folding the other ranks' partial summaries must not re-export them). */
int gs_cc_set_marking(gs_cc_t* h, int on);

/* ---- multi-GPU CombineCC (windowAll / tree reduce of partial summaries), csrc/comm.hip ----
 * One process (or thread) per GPU, one gs_comm_t per rank. Replaces the windowAll gather of the
 * partitions' window results (SummaryBulkAggregation.java:81-83) and ConnectedComponentsTree's
 * pairwise rounds (SummaryTreeReduce.java:95-123) with RCCL collectives over xGMI.
 *   gs_comm_unique_id   rank 0 makes the 128-byte RCCL unique id; the caller hands it to every
 *                       rank (torch.distributed broadcast, the job configuration, ...)
 *   gs_comm_create      every rank, concurrently: ncclCommInitRank(world, id, rank) on `device`
 *   gs_comm_create_local  `world` communicators of ONE process and device, one thread per rank
 *                       (tests of the exchange on a one-GPU box: RCCL refuses two ranks on one device)
 *   gs_cc_merge_window  after folding this rank's slice of a window: exchange this window's
 *                       partial summary (the handle needs GS_CC_TRACK_MARKS) and close the window.
 *     GS_MERGE_ALLGATHER  every rank keeps the GLOBAL summary (all-gather of deltas; every rank's
 *                         emission is the Merger's). From the second window on ONE all-gather of
 *                         slots sized from the last window's deltas (an outgrown slot costs one
 *                         more exact round, decided alike on every rank)
 *     GS_MERGE_GATHER     windowAll: deltas to rank 0, which folds them and emits
 *     GS_MERGE_TREE       log2(P) pairwise rounds to rank 0 (SummaryTreeReduce.enhance)
 *     GS_MERGE_PREFILTER  gs_cc_fold_windows only (the exchange needs the window's edges): ranks
 *                         1..P-1 keep no forest — each filters its slice of a window against the
 *                         giant bitmap rank 0 broadcasts and sends the surviving edges to rank 0,
 *                         which folds its own slice and every survivor, closes and emits (dense
 *                         ids; GS_CC_TRACK_MARKS not needed). Slices may differ in size per rank
 *                         and may be empty. The bitmap goes out after close 0 on the call's stream
 *                         (window 2's filter waits for it), later ones on a side stream over a
 *                         communicator split from this one when a handle is first bound in this
 *                         mode (collective), installed two windows later: a stale bitmap only lets
 *                         more edges through.
 *   Every rank must call it once per window with the same mode. In GATHER / TREE only rank 0's
 *   emission is the job's, and the call waits for the delta sizes. In ALLGATHER it does not wait:
 *   the sizes are checked lazily (an outgrown slot's tail round) by the next merge_window, or first
 *   thing in any call that consumes the emission or folds (stats, checksum, emit_*, find,
 *   labels_device, sync, fold*, merge, combine, reset, destroy) — gs_cc_fold_windows alone folds
 *   the next window without that wait (its merge exports before settling). */
typedef struct gs_comm gs_comm_t;
enum { GS_MERGE_ALLGATHER = 0, GS_MERGE_GATHER = 1, GS_MERGE_TREE = 2, GS_MERGE_PREFILTER = 3 };
int gs_comm_unique_id(void* id, uint64_t id_bytes);
int gs_comm_create(gs_comm_t** out, const void* unique_id, int rank, int world, int device);
int gs_comm_create_local(gs_comm_t** comms, int world, int device);
int gs_comm_destroy(gs_comm_t* comm);
/* rank, world size, payload bytes sent / received, windows merged, and speculative rounds (of the
 * all-gather, the gather and the prefilter alike) whose slot a delta or a sender's survivors
 * outgrew: each then ran one tail round, counted on every rank that took part in it */
int gs_comm_info(gs_comm_t* comm, int* rank, int* world, uint64_t* bytes_sent, uint64_t* bytes_recv, uint64_t* exchanges,
                 uint64_t* overflows);
int gs_cc_merge_window(gs_cc_t* h, gs_comm_t* comm, int mode);

/* ---- a batch of count windows in one call ----
 * SummaryBulkAggregation.run over a bounded stream (SummaryBulkAggregation.java:68-90, the Merger
 * SummaryAggregation.java:106-119): for each window of window_edges edges of src/dst (the last
 * window may be shorter) gs_cc_fold, then gs_cc_merge_window(h, comm, mode) when comm is not NULL,
 * else gs_cc_close_window — the per-window host loop run inside the library (one ABI call per batch
 * instead of two per window). After it returns, the labels are those of the last window's
 * emission; *windows_out (may be NULL) = windows folded. Stops at the first failure. With
 * GS_MERGE_PREFILTER only rank 0 folds (the others filter their slices for it); the ranks agree on
 * the call's window count (the most any rank passes, n / window_edges rounded up; one collective per
 * call) and a rank with fewer windows, or none (n == 0), runs empty ones; window_edges may differ. */
int gs_cc_fold_windows(gs_cc_t* h, gs_comm_t* comm, int mode, const void* src, const void* dst, uint64_t n,
                       uint64_t window_edges, uint64_t* windows_out);

/* ---- instrumentation ----
 * kernel ids: 0 fold (young-forest / plain k_fold launches), 1 compress (close_window), 2 merge,
 * 3 export, 4 ring (the steady k_fold_ring launches), 5 reserved (a retired steady-fold variant;
 * always 0); fold time = 0 + 4. */
enum { GS_K_FOLD = 0, GS_K_COMPRESS = 1, GS_K_MERGE = 2, GS_K_EXPORT = 3, GS_K_RING = 4, GS_K_ROUTE = 5, GS_K_COUNT = 6 };
/* enable = 0: off; 1: every kernel; GS_TIMING_MASK | (1 << GS_K_x) | ...: only those kernels
 * carry timing events (a timed launch costs ~3 us more dispatch time). Totals reset. */
enum { GS_TIMING_MASK = 0x100 };
int gs_cc_timing(gs_cc_t* h, int enable);
int gs_cc_kernel_time(gs_cc_t* h, int kernel, double* total_ms, uint64_t* launches);
/* units the timed launches of that class processed since gs_cc_timing: edges for folds and merges
 * (what each launch actually folded, after the library's internal cuts), vertex capacity per close */
int gs_cc_kernel_units(gs_cc_t* h, int kernel, uint64_t* units);

/* ---- synthetic streams on the device (definition: oracle/gen.c header) ----
 * Write ids [first, first+n) of the stream into src/dst (device pointers, id_bits wide). */
int gs_gen_rmat(void* src, void* dst, uint32_t id_bits, uint64_t first, uint64_t n, int scale,
                uint64_t seed, uint32_t ta, uint32_t tb, uint32_t tc, int scramble, void* hip_stream);
int gs_gen_er(void* src, void* dst, uint32_t id_bits, uint64_t first, uint64_t n, uint64_t nv,
              uint64_t seed, void* hip_stream);

/* ---- edge-file ingestion (ConnectedComponentsExample.java:108-119) ----
 * Parses n_bytes of text, one edge per line: Long.parseLong of fields 0 and 1 of
 * line.split("\\s") (one whitespace character between fields; trailing whitespace and fields
 * past the second ignored; a last line without '\n' counts). text: host or device; src/dst:
 * host or device, id_bits wide, capacity cap edges. *n_edges = lines parsed. A line the
 * reference would reject -> GS_ERR_INVALID, *n_edges = its 0-based index. */
int gs_parse_edges(const char* text, uint64_t n_bytes, uint32_t id_bits, void* src, void* dst, uint64_t cap,
                   uint64_t* n_edges, int device, void* hip_stream);

/* ---- streaming edge-file ingestion into a summary (ConnectedComponentsExample.java:108-119 ->
 * edges.aggregate(new ConnectedComponents<>(mergeWindowTime)), :61) ----
 * The text (gs_parse_edges' line rules) is consumed in chunks of at most chunk_bytes (0 = 64 MiB),
 * each cut after its last '
' (the partial last line carried to the next chunk), copied to the
 * device through two pinned staging buffers (the host's read / copy of chunk i+1 overlaps the parse
 * of chunk i and the folds of chunk i-1), parsed on the device into an edge ring, and folded into h
 * straight from it in count windows of window_edges edges, every window closed (the Merger's
 * emission; a last partial window is closed too). The ids never return to the host.
 * gs_cc_fold_text: text in host memory (pinned: DMA straight from it; pageable: through the pinned
 * staging) or device memory (one chunk). gs_cc_fold_file: read(2) from path into the staging.
 * h: either id width; GS_CC_SPARSE_IDS summaries take any Long id. *edges_out = edges folded; *windows_out =
 * windows closed. A line the reference rejects: GS_ERR_INVALID, every line before it folded (its
 * window left open), *edges_out = its 0-based line number. A line longer than chunk_bytes:
 * GS_ERR_CAPACITY (a read error: GS_ERR_INVALID), every whole chunk before the one holding it
 * folded (its window left open), *edges_out = the lines folded. Enqueued on h's stream like
 * gs_cc_fold_windows. on_window (may be NULL): called on the calling thread after window w's close is enqueued (w counts from 0 per call): the Merger's
 * per-window emission hook (read it with gs_cc_emit_delta / _pairs / gs_cc_checksum there); with a
 * callback every window is folded and closed by a call of its own (gs_cc_fold + gs_cc_close_window)
 * instead of in gs_cc_fold_windows batches. */
typedef void (*gs_window_fn)(void* ctx, uint64_t window);
int gs_cc_fold_text(gs_cc_t* h, const char* text, uint64_t n_bytes, uint64_t window_edges, uint64_t chunk_bytes,
                    gs_window_fn on_window, void* ctx, uint64_t* edges_out, uint64_t* windows_out);
int gs_cc_fold_file(gs_cc_t* h, const char* path, uint64_t window_edges, uint64_t chunk_bytes,
                    gs_window_fn on_window, void* ctx, uint64_t* edges_out, uint64_t* windows_out);

/* ---- BipartitenessCheck (library/BipartitenessCheck.java:38-133, summaries/Candidates.java) ----
 * A Candidates summary on the device: union-find with a parity bit per vertex. ids in
 * [0, vertex_capacity), vertex_capacity <= 2^31 - 1, id_bits 32 or 64. The emission of a
 * bipartite summary = every vertex with its component key (the component's minimum id) and its
 * sign (true iff on the key vertex's side); a summary that has seen an odd cycle is failed for
 * good (Candidates.fail(): "(false,{})"). Self-loops only add their vertex (edgeToCandidate).
 *   gs_bip_create / _reset     new Candidates(true)                       (Candidates.java:30-33)
 *   gs_bip_fold / _fold_pairs  updateFunction.foldEdges over a batch      (BipartitenessCheck.java:93-95)
 *   gs_bip_merge               combineFunction.reduce: into.merge(from)   (BipartitenessCheck.java:121-124)
 *   gs_bip_close_window        the Merger's per-window emission           (SummaryAggregation.java:106-119)
 *   gs_bip_status / _checksum  getSuccess() (Candidates.java:40-42), sizes, and
 *                              sum over v of splitmix64(v ^ splitmix64(((key << 1) | sign) ^ 0xD1B54A32D192ED03))
 *   gs_bip_emit_pairs          (vertex, key, sign) ordered by vertex      (Candidates.getMap(), :44-46)
 *   gs_bip_restore             restoreState: the summary becomes a snapshot's — getSuccess() and
 *                              the n entries gs_bip_emit_pairs wrote (any order; host or device
 *                              arrays of the handle's id width)           (SummaryAggregation.java:121-135)
 * GS_BIP_REFERENCE_LITERAL (gs_bip_create_ex): the reference's Candidates rule as written
 * (Candidates.java:77-192) instead of its intended semantics, for callers that need the reference's
 * emissions on multi-window / multi-partition streams: a merge writes an input component under
 * min(input key, lowest overlapping key) and removes only the other overlapping components (so a
 * vertex may sit in several components), drops the result of their inner merges (:130), keeps the
 * receiving side's signs, and skips components with an equal vertex set. The rule is sequential:
 * one workgroup applies it edge after edge (csrc/bip_literal.hpp), for parity, not throughput.
 * State: at most entry_capacity component memberships made between resets (0: 16 x
 * vertex_capacity; GS_ERR_CAPACITY past it). Such summaries merge only with each other;
 * gs_bip_status / _checksum count (component, vertex) entries; gs_bip_emit_pairs writes every
 * entry ordered by vertex, then key; close_window is a no-op; a place where the reference's
 * merge would throw (an empty mergeBy list, :156) fails the call with GS_ERR_INVALID; gs_bip_restore
 * loads the entries as they are (components sharing vertices included). An intended-semantics
 * summary is restored from one parity edge per vertex (GS_ERR_INVALID for entries no bipartite
 * summary emits: a key outside its component, a component of one side only). */
typedef struct gs_bip gs_bip_t;
enum { GS_BIP_REFERENCE_LITERAL = 1 };
int gs_bip_create(gs_bip_t** out, uint64_t vertex_capacity, uint32_t id_bits, int device);
int gs_bip_create_ex(gs_bip_t** out, uint64_t vertex_capacity, uint32_t id_bits, int device, uint32_t flags,
                     uint64_t entry_capacity);
int gs_bip_destroy(gs_bip_t* h);
int gs_bip_reset(gs_bip_t* h);
int gs_bip_set_stream(gs_bip_t* h, void* hip_stream);
int gs_bip_sync(gs_bip_t* h);
int gs_bip_fold(gs_bip_t* h, const void* src, const void* dst, uint64_t n);
int gs_bip_fold_pairs(gs_bip_t* h, const void* pairs, uint64_t n);
int gs_bip_merge(gs_bip_t* into, gs_bip_t* from);
int gs_bip_close_window(gs_bip_t* h);
int gs_bip_status(gs_bip_t* h, int* bipartite, uint64_t* n_vertices, uint64_t* n_components);
int gs_bip_checksum(gs_bip_t* h, uint64_t* checksum, int* bipartite, uint64_t* n_vertices, uint64_t* n_components);
int gs_bip_emit_pairs(gs_bip_t* h, void* vertices, void* keys, uint8_t* signs, uint64_t cap, uint64_t* n_out);
int gs_bip_restore(gs_bip_t* h, int bipartite, const void* vertices, const void* keys, const uint8_t* signs, uint64_t n);

/* ---- WindowTriangles (example/WindowTriangles.java:60-65, :82-139) ----
 * Exact triangle counts of edge windows: slice(window, ALL) -> GenerateCandidateEdges ->
 * CountTriangles -> timeWindowAll.sum. The count of a window is the number of triangles of its
 * simple undirected graph: repeated edges and both directions count once, every triangle is found
 * once (at its lowest vertex of the orientation). Self-loops are ignored (with one the reference's
 * count depends on HashSet iteration order). Dense ids in [0, vertex_capacity), vertex_capacity
 * <= 2^32, id_bits 32 or 64. A handle holds no summary between calls, only scratch memory.
 *   flags: GS_TRI_ORIENT_BY_ID   orient edges low id -> high id (the reference's own rule, "IDs
 *          larger than the vertex ID"); default low (degree, id) -> high (degree, id), under which
 *          no out-row holds more than sqrt(2 m) of a window's m simple edges.
 *   gs_tri_count_windows  every window of window_edges edges (the last may be shorter):
 *          counts[w] = triangles of window w (host array of cap entries); *n_windows =
 *          ceil(n / window_edges); cap < that: GS_ERR_CAPACITY, nothing counted. One host wait,
 *          at the end. src/dst host or device, id_bits wide, as gs_cc_fold. n == 0: GS_OK,
 *          *n_windows = 0.
 *   gs_tri_count_local    one window; local (nullable, host or device, vertex_capacity uint64
 *          entries) = triangles per vertex (for a stream without repeated edges: the final
 *          per-vertex counters of ExactTriangleCount.java); *triangles = the total,
 *          *simple_edges (nullable) = distinct undirected edges without self-loops.
 * An id outside [0, vertex_capacity): GS_ERR_RANGE, and the call reports no count. */
typedef struct gs_tri gs_tri_t;
enum { GS_TRI_ORIENT_BY_ID = 1 };
int gs_tri_create(gs_tri_t** out, uint64_t vertex_capacity, uint32_t id_bits, int device, uint32_t flags);
int gs_tri_destroy(gs_tri_t* h);              /* NULL is GS_OK, like gs_cc_destroy */
int gs_tri_set_stream(gs_tri_t* h, void* hip_stream);
int gs_tri_get_stream(gs_tri_t* h, void** hip_stream);
int gs_tri_sync(gs_tri_t* h);
int gs_tri_count_windows(gs_tri_t* h, const void* src, const void* dst, uint64_t n, uint64_t window_edges,
                         uint64_t* counts, uint64_t cap, uint64_t* n_windows);
int gs_tri_count_local(gs_tri_t* h, const void* src, const void* dst, uint64_t n,
                       uint64_t* local, uint64_t* triangles, uint64_t* simple_edges);

/* ---- streaming degrees and DegreeDistribution, with edge deletions ----
 * (SimpleEdgeStream.getDegrees / getInDegrees / getOutDegrees, SimpleEdgeStream.java:413-478;
 *  example/DegreeDistribution.java:70-132, the reference's consumer of EventType)
 * The summary: degree[v] of every vertex with degree > 0, and count[d] = vertices of degree d.
 * An event (src, dst, add) is two vertex events in stream order, src then dst (GS_DEG_OUT keeps
 * only sources, GS_DEG_IN only targets; neither or both: both). A vertex event changes the degree
 * x of its vertex to max(x + change, 0), change = +1 | -1, absent = 0: a deletion at an absent
 * vertex is ignored, a vertex whose degree reaches 0 leaves the map (VertexDegreeCounts.flatMap).
 * A self-loop adds 2 (1 with GS_DEG_IN or GS_DEG_OUT). The library works in count windows: after a
 * window the summary equals the reference's maps after the same prefix of the stream, for any
 * stream, one that deletes more than was added included. Dense ids in [0, vertex_capacity),
 * vertex_capacity <= 2^32 - 1, id_bits 32 or 64. add: nullable uint8 array (1 = addition, 0 =
 * deletion; NULL = all additions). src / dst / add host or device, as for gs_cc_fold.
 * Per-window emissions (the reference emits per record):
 *   degree delta        the vertices whose degree after the window differs from before it, with
 *                       their new degree (0 = removed), ordered by vertex
 *   distribution delta  the degree keys whose count after the window differs from before it, with
 *                       their new count (may be 0), ordered by degree
 * Both are the reference's LAST record of that key within the window, for keys with a net change.
 * The reference's records for keys that end the window where they began are not reproduced. With
 * one-event windows the deltas are the reference's records (DegreeDistributionITCase, TestGetDegrees).
 *   flags: GS_DEG_OUT, GS_DEG_IN (above). Two paths compute a window, with equal results:
 *          GS_DEG_SORT_ALL: every vertex event takes the exact path (sort by vertex and position,
 *          ordered segmented composition); GS_DEG_COUNT: the counting path (one atomic add per
 *          vertex event on a per-vertex accumulator, plain sum at the close), which sends only the
 *          events of vertices a window could clamp through the exact path. With neither flag the
 *          library takes the one measured faster, which is sort-everything.
 *   dense_degrees: count[d] is a dense array for d < dense_degrees (0 = 65536), a hash table of
 *          at most 2^20 slots above it.
 *   gs_deg_fold_window   one window: fold and close.
 *   gs_deg_fold_windows  every window of window_edges events (the last may be shorter); one
 *          gs_deg_window_stats per window into the host array stats (cap entries); *n_windows =
 *          ceil(n / window_edges); cap < that: GS_ERR_CAPACITY, nothing folded; n == 0: GS_OK, 0
 *          windows. One host wait, at the end; with GS_DEG_COUNT a window with deletions (add !=
 *          NULL) waits once more, for a small read: the events of the vertices it could clamp.
 *   gs_deg_stats         the same numbers for the current summary. checksum = sum mod 2^64 over
 *          vertices with degree > 0 of splitmix64(v ^ splitmix64(degree ^ 0xD1B54A32D192ED03)).
 *   gs_deg_emit_degrees / _degrees_delta       (vertex, degree) ordered by vertex; vertices id_bits
 *          wide, degrees uint32; host or device arrays of cap entries; *n_out = the number of
 *          entries; cap < that: GS_ERR_CAPACITY, nothing written.
 *   gs_deg_emit_distribution / _distribution_delta   (degree, count) ordered by degree; uint32 /
 *          uint64. The deltas are those of the last window folded (of a gs_deg_fold_windows call:
 *          its last window); empty after gs_deg_reset / gs_deg_restore.
 *   gs_deg_find          degrees[i] = degree of ids[i], 0 for an absent vertex.
 *   gs_deg_restore       the summary becomes a snapshot's: the n pairs gs_deg_emit_degrees wrote, in
 *          any order; distribution, statistics and checksum are rebuilt on the device (the Merger's
 *          checkpoint, as gs_bip_restore). A repeated vertex or a degree of 0: GS_ERR_INVALID; an
 *          id outside the capacity: GS_ERR_RANGE; the summary is unchanged then.
 * Failures: an id outside [0, vertex_capacity) in a window: GS_ERR_RANGE; that window and the later
 * ones of the call are not folded and the summary is as after the last window before it. Limits:
 * degrees are 32 bits wide: a call is refused with GS_ERR_CAPACITY, before anything is folded, when
 * (largest restored degree) + 2 x (events folded since the last reset or restore, this call
 * included) could pass 2^32 - 1; likewise when more than (table slots) / 4 distinct degrees >=
 * dense_degrees are possible. A window holds at most 2^30 - 1 events; vertex, position and sign
 * must fit a 64-bit sort key (GS_ERR_UNSUPPORTED: capacity above 2^31 with windows above 2^29). */
typedef struct gs_deg gs_deg_t;
enum { GS_DEG_OUT = 1, GS_DEG_IN = 2, GS_DEG_SORT_ALL = 4, GS_DEG_COUNT = 8 };
typedef struct gs_deg_window_stats {
    uint64_t n_vertices;        /* vertices with degree > 0 */
    uint64_t n_degrees;         /* degree keys with count > 0 */
    uint64_t max_degree;
    uint64_t checksum;
} gs_deg_window_stats;
int gs_deg_create(gs_deg_t** out, uint64_t vertex_capacity, uint32_t id_bits, int device, uint32_t flags, uint32_t dense_degrees);
int gs_deg_destroy(gs_deg_t* h);              /* NULL is GS_OK */
int gs_deg_reset(gs_deg_t* h);
int gs_deg_set_stream(gs_deg_t* h, void* hip_stream);
int gs_deg_get_stream(gs_deg_t* h, void** hip_stream);
int gs_deg_sync(gs_deg_t* h);
int gs_deg_fold_window(gs_deg_t* h, const void* src, const void* dst, const uint8_t* add, uint64_t n);
int gs_deg_fold_windows(gs_deg_t* h, const void* src, const void* dst, const uint8_t* add, uint64_t n, uint64_t window_edges,
                        gs_deg_window_stats* stats, uint64_t cap, uint64_t* n_windows);
int gs_deg_stats(gs_deg_t* h, gs_deg_window_stats* stats);
/* since create: windows folded, those that took the exact path, vertex events, those that were sorted (any may be NULL) */
int gs_deg_path_counts(gs_deg_t* h, uint64_t* windows, uint64_t* exact_windows, uint64_t* vertex_events, uint64_t* exact_events);
int gs_deg_emit_degrees(gs_deg_t* h, void* vertices, uint32_t* degrees, uint64_t cap, uint64_t* n_out);
int gs_deg_emit_degrees_delta(gs_deg_t* h, void* vertices, uint32_t* degrees, uint64_t cap, uint64_t* n_out);
int gs_deg_emit_distribution(gs_deg_t* h, uint32_t* degrees, uint64_t* counts, uint64_t cap, uint64_t* n_out);
int gs_deg_emit_distribution_delta(gs_deg_t* h, uint32_t* degrees, uint64_t* counts, uint64_t cap, uint64_t* n_out);
int gs_deg_find(gs_deg_t* h, const void* ids, uint32_t* degrees, uint64_t n);
int gs_deg_restore(gs_deg_t* h, const void* vertices, const uint32_t* degrees, uint64_t n);

/* ---- neighbourhood slices: per-vertex window aggregates over edge values ----
 * (SimpleEdgeStream.slice(size, direction) -> SnapshotStream, SimpleEdgeStream.java:135-167;
 *  reduceOnEdges / foldNeighbors / applyOnNeighbors, SnapshotStream.java:61-131)
 * A count window of n edges (s, d, x), x an int64 edge value (the reference's Long), becomes a
 * list of entries (key, neighbour, value):
 *   GS_SLICE_OUT  one per edge: (s, d, x)
 *   GS_SLICE_IN   one per edge: (d, s, x)                     (reverse())
 *   GS_SLICE_ALL  two per edge: (s, d, x) at position 2i, then (d, s, x) at 2i + 1   (undirected())
 * A self-loop (u, u, x) gives u two entries under ALL and one otherwise. The row of a vertex is its
 * entries IN ARRIVAL ORDER (a keyed window keeps arrival order); a vertex has a row only if it has
 * an entry in that window. Nothing is kept between windows: the handle holds the last window's
 * slice and scratch memory. Dense ids in [0, vertex_capacity), vertex_capacity <= 2^32, id_bits 32
 * or 64, as gs_tri_*. Sparse Long ids and floating-point values are out of scope (a float sum
 * depends on the order of its terms). Records are emitted ordered by vertex (the reference emits in
 * no defined order).
 *   op: reduceOnEdges emits one (vertex, value) per row, the left-to-right reduction of the row's
 *          values; a row of one entry yields its value unchanged.
 *          GS_SLICE_SUM    two's-complement wrap, as Java long (foldNeighbors with a summing fold)
 *          GS_SLICE_MIN / GS_SLICE_MAX   signed
 *          GS_SLICE_COUNT  entries of the row; the values are ignored and may be absent
 *          GS_SLICE_FIRST / GS_SLICE_LAST   the reducers (a, b) -> a and (a, b) -> b
 *   src / dst / val: host or device pointers, as for gs_cc_fold; src / dst id_bits wide. val == NULL
 *          is allowed with GS_SLICE_COUNT only: any other op on such a slice is GS_ERR_INVALID, and
 *          gs_slice_rows then writes no values, so its values argument must be NULL too.
 *   gs_slice_window   builds the slice of one window (it copies what it needs: the caller's arrays
 *          are free on return). n == 0: GS_OK, an empty slice.
 *   gs_slice_reduce   reads the slice the last gs_slice_window built; may be called repeatedly
 *          with different ops. vertices (id_bits wide) and values: host or device arrays of cap
 *          entries; *n_out = the number of rows; cap < that: GS_ERR_CAPACITY, nothing written.
 *   gs_slice_rows     the same slice as CSR, what applyOnNeighbors iterates: vertices[nv],
 *          offsets[nv + 1], neighbours[ne] (id_bits wide), values[ne]; row r is
 *          offsets[r] .. offsets[r + 1], in arrival order. Host or device arrays; a capacity too
 *          small: GS_ERR_CAPACITY, nothing written, *n_vertices / *n_entries report the need.
 *   gs_slice_stats    n_vertices, n_entries, max_row (the longest row) and checksum = sum mod 2^64
 *          over rows of splitmix64(vertex ^ splitmix64(value ^ 0xD1B54A32D192ED03)), value = the
 *          row's reduction under op.
 *   gs_slice_reduce_windows   every window of window_edges edges (the last may be shorter), with
 *          one host wait, at the end. The records are written concatenated (host or device arrays
 *          of cap entries); window w is window_offsets[w] .. window_offsets[w + 1]. window_offsets
 *          (cap_windows + 1 entries) and stats (cap_windows entries, nullable) are host arrays.
 *          *n_windows = ceil(n / window_edges); cap_windows < that: GS_ERR_CAPACITY, nothing is
 *          run. Records that outgrow cap: GS_ERR_CAPACITY, nothing is written past cap and the
 *          outputs are unspecified. Afterwards the handle holds the call's last window.
 * An id outside [0, vertex_capacity): GS_ERR_RANGE; that window and the later ones of the call
 * report nothing, and the handle then holds an empty slice. An unknown op or direction:
 * GS_ERR_INVALID. Limits: a window holds at most 2^30 - 1 edges (positions are 32 bits and the sort
 * counts entries in an int); above that GS_ERR_UNSUPPORTED, before anything runs. */
typedef struct gs_slice gs_slice_t;
enum { GS_SLICE_OUT = 0, GS_SLICE_IN = 1, GS_SLICE_ALL = 2 };
enum { GS_SLICE_SUM = 0, GS_SLICE_MIN = 1, GS_SLICE_MAX = 2, GS_SLICE_COUNT = 3, GS_SLICE_FIRST = 4, GS_SLICE_LAST = 5 };
typedef struct gs_slice_window_stats {
    uint64_t n_vertices;        /* rows of the window */
    uint64_t n_entries;
    uint64_t max_row;           /* entries of the longest row */
    uint64_t checksum;
} gs_slice_window_stats;
int gs_slice_create(gs_slice_t** out, uint64_t vertex_capacity, uint32_t id_bits, int device, uint32_t direction);
int gs_slice_destroy(gs_slice_t* h);          /* NULL is GS_OK */
int gs_slice_set_stream(gs_slice_t* h, void* hip_stream);
int gs_slice_get_stream(gs_slice_t* h, void** hip_stream);
int gs_slice_sync(gs_slice_t* h);
int gs_slice_window(gs_slice_t* h, const void* src, const void* dst, const int64_t* val, uint64_t n);
int gs_slice_reduce(gs_slice_t* h, int op, void* vertices, int64_t* values, uint64_t cap, uint64_t* n_out);
int gs_slice_rows(gs_slice_t* h, void* vertices, uint64_t* offsets, void* neighbours, int64_t* values,
                  uint64_t cap_vertices, uint64_t cap_entries, uint64_t* n_vertices, uint64_t* n_entries);
int gs_slice_stats(gs_slice_t* h, int op, gs_slice_window_stats* stats);
int gs_slice_reduce_windows(gs_slice_t* h, const void* src, const void* dst, const int64_t* val, uint64_t n,
                            uint64_t window_edges, int op, void* vertices, int64_t* values, uint64_t cap,
                            uint64_t* window_offsets, gs_slice_window_stats* stats, uint64_t cap_windows,
                            uint64_t* n_windows);

const char* gs_last_error(void);
int gs_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GSGPU_H */
