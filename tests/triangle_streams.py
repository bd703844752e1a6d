"""Seeded structured edge windows for the triangle counter (gs_tri_*) and a reference that does not
share its method.

``sparse_count`` counts by sparse matrix products over the strictly upper-triangular adjacency
matrix (ids compressed first, so the capacity never enters the cost); tri.hip counts by
intersecting sorted out-rows of an oriented adjacency. ``sorted_adjacency_count``
(triangles_oracle.py) orients by degree exactly as tri.hip does, so it is not the reference here.

Each family reaches a region of tri.hip that needs a size the random streams never have:

* ``wide_grid``       21 id bits (keys above 2^32) and more than 2^20 edges and simple edges (a
                      second trip of every grid-stride loop);
* ``many_long_rows``  more than 4,096 rows longer than kShortRow with the long-row grid at its cap
                      (a k_tri_long workgroup serves a second row);
* ``tile_edges``      a row of kTile - 1, kTile, kTile + 1, 2 kTile and 2 kTile + 1 ids whose matches
                      sit in another tile than the b they are found from;
* ``regular_long``    long rows under the degree orientation (every degree equal: ties by id);
* ``wide_windows``    ``wide_grid`` in windows, a window of self-loops only, then a path.

Every family shuffles its edges and reverses about half of them unless it says otherwise."""
import functools
import json
import os

import numpy as np
import scipy.sparse as sp

KTILE = 8192                       # tri.hip kTile
KSHORT = 64                        # tri.hip kShortRow
MAX_BLOCKS = 4096                  # tri.hip kTriMaxBlocks
THREADS = 256                      # tri.hip kTriThreads
GRID_SPAN = MAX_BLOCKS * THREADS   # items one trip of a grid-stride loop covers

WIDE_CAPACITY = (1 << 20) + 3
TILE_SIZES = (KTILE - 1, KTILE, KTILE + 1, 2 * KTILE, 2 * KTILE + 1)


def bits_for(capacity):
    """Id bits of a key: tri.hip's rule in gs_tri_create."""
    b = 1
    while b < 32 and (1 << b) < capacity:
        b += 1
    return b


# ---- the reference ----
def sparse_count(src, dst):
    """(total, ids, local, simple_edges): the triangles of the simple undirected graph of the
    edges, the ascending ids of its vertices, per-vertex counts in that order, and its edge count.

    U is the strictly upper-triangular 0/1 matrix over the compressed ids. (U U)[a, c] counts the b
    with a < b < c adjacent to both, so T = (U U) o U holds every triangle a < b < c once, at
    (a, c): its row sums are the counts of the smallest corners, its column sums those of the
    largest. M = (U^T U) o U holds it at (b, c): its row sums are the counts of the middle ones
    (masked_gram: the same matrix without the unmasked product)."""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    keep = src != dst
    lo, hi = np.minimum(src[keep], dst[keep]), np.maximum(src[keep], dst[keep])
    if lo.size == 0:
        return 0, np.empty(0, dtype=np.int64), np.empty(0, dtype=np.uint64), 0
    ids, inv = np.unique(np.concatenate([lo, hi]), return_inverse=True)
    nv = ids.size
    pair = np.unique(inv[:lo.size].astype(np.int64) * nv + inv[lo.size:])
    r, c = pair // nv, pair % nv
    U = sp.csr_matrix((np.ones(pair.size, dtype=np.int64), (r, c)), shape=(nv, nv))
    T = (U @ U).multiply(U)
    M = masked_gram(U)
    local = (np.asarray(T.sum(axis=1)).ravel() + np.asarray(T.sum(axis=0)).ravel()
             + np.asarray(M.sum(axis=1)).ravel())
    return int(T.sum()), ids, local.astype(np.uint64), int(pair.size)


def masked_gram(U, chunk=1 << 18, direct=None):
    """(U^T U) o U, evaluated at U's entries only: entry (b, c) is the dot product of columns b and
    c of U. The product U^T U itself has a full L x L block under a vertex that is the smaller end
    of L edges (3 GB for tile_edges' hub), none of which survives the mask but U's own entries."""
    r, c = U.nonzero()
    out_deg = np.diff(U.indptr).astype(np.int64)
    in_deg = np.bincount(c, minlength=U.shape[0]).astype(np.int64)
    if direct is None:
        direct = int((out_deg * out_deg).sum()) <= 4 * int((in_deg[r] + in_deg[c]).sum())
    if direct:
        return (U.T @ U).multiply(U).tocsr()               # the product is no larger than the work below
    Ut = U.T.tocsr()
    vals = np.empty(r.size, dtype=np.int64)
    for lo in range(0, r.size, chunk):
        vals[lo:lo + chunk] = np.asarray(Ut[r[lo:lo + chunk]].multiply(Ut[c[lo:lo + chunk]]).sum(axis=1)).ravel()
    return sp.csr_matrix((vals, (r, c)), shape=U.shape)


def scatter_local(ids, local, capacity):
    """The reference's per-vertex counts as the capacity-long array gs_tri_count_local fills."""
    out = np.zeros(capacity, dtype=np.uint64)
    out[ids] = local
    return out


def out_row_lengths(src, dst, capacity, by_degree):
    """Out-row length per vertex under tri.hip's two orientation rules (low (degree, id) -> high,
    or low id -> high id): what decides which rows k_tri_long takes."""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    keep = src != dst
    lo, hi = np.minimum(src[keep], dst[keep]), np.maximum(src[keep], dst[keep])
    pair = np.unique(lo * np.int64(capacity) + hi)
    lo, hi = pair // capacity, pair % capacity
    if by_degree:
        deg = np.bincount(lo, minlength=capacity) + np.bincount(hi, minlength=capacity)
        a = np.where(deg[lo] > deg[hi], hi, lo)
    else:
        a = lo
    return np.bincount(a, minlength=capacity)


# ---- the families ----
def _mix(src, dst, rng, reverse=True):
    """Shuffled edge order, about half of the edges reversed."""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    order = rng.permutation(src.size)
    src, dst = src[order], dst[order]
    if reverse:
        flip = rng.random(src.size) < 0.5
        src, dst = np.where(flip, dst, src), np.where(flip, src, dst)
    return np.ascontiguousarray(src), np.ascontiguousarray(dst)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


GRID_R = GRID_C = 600


@functools.lru_cache(maxsize=None)
def wide_grid(seed=20):
    """The triangulated 600 x 600 grid (right, down and down-right edges) under a seeded injection
    into [0, 2^20 + 3) that uses ids 0 and capacity - 1, plus 2^18 repeated edges (half reversed)
    and 1,000 self-loops. Returns (src, dst, capacity, ids_of_grid), ids_of_grid[r * C + c] being
    the id of grid vertex (r, c)."""
    rng = np.random.default_rng(seed)
    R, C = GRID_R, GRID_C
    cap = WIDE_CAPACITY
    inner = rng.choice(cap - 2, size=R * C - 2, replace=False) + 1          # distinct, in [1, cap - 2]
    ident = rng.permutation(np.concatenate([inner, [0, cap - 1]]).astype(np.int64))
    v = np.arange(R * C, dtype=np.int64).reshape(R, C)
    s = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel(), v[:-1, :-1].ravel()])
    d = np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel(), v[1:, 1:].ravel()])
    s, d = ident[s], ident[d]
    again = rng.integers(0, s.size, size=1 << 18)
    loops = ident[rng.integers(0, R * C, size=1000)]
    src, dst = _mix(np.concatenate([s, s[again], loops]), np.concatenate([d, d[again], loops]), rng)
    _frozen(src, dst, ident)
    return src, dst, cap, ident


def wide_grid_total():
    return 2 * (GRID_R - 1) * (GRID_C - 1)


WIDE_GRID_SIMPLE = GRID_R * (GRID_C - 1) + (GRID_R - 1) * GRID_C + (GRID_R - 1) * (GRID_C - 1)   # 1,077,601

N_HUBS, N_LEAVES, HUB_FAN = 4200, 130, 66


@functools.lru_cache(maxsize=None)
def many_long_rows(seed=21):
    """Hubs 0..4,199, hub h joined to the 66 leaves 4200 + (7 h + j) % 130; the 130 leaves form a
    clique. Returns (src, dst, capacity)."""
    rng = np.random.default_rng(seed)
    h = np.repeat(np.arange(N_HUBS, dtype=np.int64), HUB_FAN)
    j = np.tile(np.arange(HUB_FAN, dtype=np.int64), N_HUBS)
    leaf = N_HUBS + (7 * h + j) % N_LEAVES
    a, b = np.triu_indices(N_LEAVES, 1)
    src, dst = _mix(np.concatenate([h, N_HUBS + a]), np.concatenate([leaf, N_HUBS + b]), rng)
    _frozen(src, dst)
    return src, dst, N_HUBS + N_LEAVES


def many_long_rows_total():
    return N_HUBS * (HUB_FAN * (HUB_FAN - 1) // 2) + N_LEAVES * (N_LEAVES - 1) * (N_LEAVES - 2) // 6


@functools.lru_cache(maxsize=None)
def tile_edges(L, seed=22):
    """Hub 0, leaves 1..L, leaf edges i - i + 1 and i - i + 8,193. Under the id orientation the
    hub's row is 1..L; the triangle (0, i, i + 8193) is found from b = i with w = i + 8193, which
    lies in another tile than b. Returns (src, dst, capacity)."""
    rng = np.random.default_rng(seed + L)
    leaves = np.arange(1, L + 1, dtype=np.int64)
    far = leaves[leaves + KTILE + 1 <= L]
    src, dst = _mix(np.concatenate([np.zeros(L, dtype=np.int64), leaves[:-1], far]),
                    np.concatenate([leaves, leaves[1:], far + KTILE + 1]), rng)
    _frozen(src, dst)
    return src, dst, L + 1


def tile_edges_total(L):
    return (L - 1) + max(L - (KTILE + 1), 0)


CIRC_N, CIRC_K, CLIQUE = 4099, 80, 200


@functools.lru_cache(maxsize=None)
def regular_long(with_clique, seed=23):
    """The circulant on 4,099 vertices with offsets 1..80 (every degree 160: the degree orientation
    falls back to id order, and the out-rows of the low ids hold up to 160 ids); with_clique adds a
    disjoint 200-clique on the ids above it. Returns (src, dst, capacity)."""
    rng = np.random.default_rng(seed + int(with_clique))
    v = np.repeat(np.arange(CIRC_N, dtype=np.int64), CIRC_K)
    off = np.tile(np.arange(1, CIRC_K + 1, dtype=np.int64), CIRC_N)
    s, d, cap = v, (v + off) % CIRC_N, CIRC_N
    if with_clique:
        a, b = np.triu_indices(CLIQUE, 1)
        s, d, cap = np.concatenate([s, CIRC_N + a]), np.concatenate([d, CIRC_N + b]), CIRC_N + CLIQUE
    src, dst = _mix(s, d, rng)
    _frozen(src, dst)
    return src, dst, cap


def regular_long_total(with_clique):
    """n > 3 k: a triangle spans an arc of a + b <= k steps (a, b >= 1) from its first vertex."""
    t = CIRC_N * (CIRC_K * (CIRC_K - 1) // 2)
    return t + (CLIQUE * (CLIQUE - 1) * (CLIQUE - 2) // 6 if with_clique else 0)


WIDE_WINDOW = 1 << 18


@functools.lru_cache(maxsize=None)
def wide_windows(seed=24):
    """wide_grid's stream in windows of 2^18 edges (the last one filled up with self-loops), a
    window of self-loops only, then a short window: a path in random id order over 3,000 of the
    grid's ids, 0 and capacity - 1 among them. Returns (src, dst, capacity, window_edges)."""
    rng = np.random.default_rng(seed)
    gs, gd, cap, ident = wide_grid()
    W = WIDE_WINDOW
    pad = -gs.size % W
    loops = ident[rng.integers(0, ident.size, size=pad + W)]
    walk = rng.permutation(np.concatenate([rng.choice(ident[(ident != 0) & (ident != cap - 1)], 2998, replace=False),
                                           [0, cap - 1]]))
    src = np.concatenate([gs, loops, walk[:-1]])
    dst = np.concatenate([gd, loops, walk[1:]])
    _frozen(src, dst)
    return src, dst, cap, W


def known_answer():
    """The reference's 19-edge known answer as one window per entry: [(src, dst, count)]."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "window_triangles_kat.json")
    with open(path) as f:
        k = json.load(f)
    e = np.asarray(k["edges"], dtype=np.int64)
    wid = e[:, 2] // k["window_ms"]
    return [(e[wid == w, 0], e[wid == w, 1], int(c)) for w, (c, _) in zip(np.unique(wid), k["expected"])]


# ---- references, computed once and shared ----
def reference(name, arg=None):
    """(total, local scattered over the capacity, simple edges) of a one-window family."""
    return _reference(name, arg)


@functools.lru_cache(maxsize=None)
def _reference(name, arg):
    src, dst, cap = FAMILIES[name](arg)[:3] if arg is not None else FAMILIES[name]()[:3]
    total, ids, local, m = sparse_count(src, dst)
    full = scatter_local(ids, local, cap)
    full.setflags(write=False)
    return total, full, m


@functools.lru_cache(maxsize=None)
def window_reference():
    """Per-window (total, simple edges) of wide_windows."""
    src, dst, cap, W = wide_windows()
    out = []
    for lo in range(0, src.size, W):
        total, _, _, m = sparse_count(src[lo:lo + W], dst[lo:lo + W])
        out.append((total, m))
    return tuple(out)


WIDE_SPLIT = 1 << 20


@functools.lru_cache(maxsize=None)
def wide_grid_split_reference():
    """Totals of wide_grid's stream cut at 2^20 edges (two windows)."""
    src, dst = wide_grid()[:2]
    return (sparse_count(src[:WIDE_SPLIT], dst[:WIDE_SPLIT])[0], sparse_count(src[WIDE_SPLIT:], dst[WIDE_SPLIT:])[0])


FAMILIES = {"wide_grid": wide_grid, "many_long_rows": many_long_rows, "tile_edges": tile_edges,
            "regular_long": regular_long}
