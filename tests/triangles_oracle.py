"""CPU oracles for the triangle counts (numpy only).

* ``literal_window_count``  the reference's GenerateCandidateEdges + CountTriangles
  (example/WindowTriangles.java:82-139) restated step by step for one window;
* ``dense_count``           trace(A^3) / 6 and diag(A^3) / 2 of the window's simple graph;
* ``sorted_adjacency_count`` the same numbers from sorted adjacency rows, for sizes at which a
  dense matrix is too big.
"""
from collections import defaultdict

import numpy as np


def drop_self_loops(src, dst):
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    keep = src != dst
    return src[keep], dst[keep]


def literal_window_count(src, dst):
    """One window through the reference's two functions; the sum timeWindowAll.sum(0) emits.

    slice(window, ALL) hands every vertex one (neighbour) tuple per incident edge, in either
    direction. GenerateCandidateEdges emits (vertex, neighbour, false) for each, then for the
    distinct neighbour ids n[0..k) every (n[i], n[j], true) with i < k - 1, i <= j < k and both ids
    larger than the vertex. CountTriangles groups by (f0, f1) and emits the group's number of
    candidates when the group holds an edge tuple. The ids are walked in ascending order here;
    Java walks a HashSet. Without self-loops the order cannot change the sum (a (x, x) candidate
    never meets an edge tuple, and both (x, y) and (y, x) groups hold edge tuples), with one it
    can, so callers remove self-loops first (drop_self_loops)."""
    src = np.asarray(src, dtype=np.int64).tolist()
    dst = np.asarray(dst, dtype=np.int64).tolist()
    neighbours = defaultdict(list)
    for u, v in zip(src, dst):
        neighbours[u].append(v)
        neighbours[v].append(u)
    edges = defaultdict(int)
    candidates = defaultdict(int)
    for vertex, nbrs in neighbours.items():
        for x in nbrs:
            edges[(vertex, x)] += 1
        ids = sorted(set(nbrs))
        for i in range(len(ids) - 1):
            for j in range(i, len(ids)):
                if ids[i] > vertex and ids[j] > vertex:
                    candidates[(ids[i], ids[j])] += 1
    return sum(c for key, c in candidates.items() if edges.get(key, 0) > 0)


def simple_edges(src, dst):
    """The distinct undirected edges (lo, hi), lo < hi, of the window."""
    src, dst = drop_self_loops(src, dst)
    lo, hi = np.minimum(src, dst), np.maximum(src, dst)
    if lo.size == 0:
        return lo, hi
    pairs = np.unique(np.stack([lo, hi], axis=1), axis=0)
    return pairs[:, 0], pairs[:, 1]


def dense_count(src, dst, nv):
    """(triangles, per-vertex triangles) = (trace(A^3) / 6, diag(A^3) / 2)."""
    lo, hi = simple_edges(src, dst)
    a = np.zeros((nv, nv), dtype=np.float64)           # exact: every entry of A^3 is far below 2^53
    a[lo, hi] = 1.0
    a[hi, lo] = 1.0
    d = np.einsum("ij,ji->i", a @ a, a)
    local = np.rint(d / 2).astype(np.uint64)
    return int(round(d.sum() / 6)), local


def sorted_adjacency_count(src, dst, nv):
    """The same from rows: edges directed low (degree, id) -> high, rows sorted; a triangle is an
    edge a -> b with a common out-neighbour w, found by looking (b, w) up among the sorted edges."""
    lo, hi = simple_edges(src, dst)
    local = np.zeros(nv, dtype=np.uint64)
    if lo.size == 0:
        return 0, local
    deg = np.bincount(lo, minlength=nv) + np.bincount(hi, minlength=nv)
    flip = deg[lo] > deg[hi]
    a = np.where(flip, hi, lo)
    b = np.where(flip, lo, hi)
    order = np.lexsort((b, a))
    a, b = a[order], b[order]
    key = a * np.int64(nv) + b                         # ascending
    start = np.searchsorted(a, np.arange(nv), side="left")
    out = np.bincount(a, minlength=nv)
    # every wedge a -> b, a -> w: edge e paired with each entry of a's row
    reps = out[a]
    e = np.repeat(np.arange(a.size), reps)
    within = np.arange(reps.sum()) - np.repeat(np.cumsum(reps) - reps, reps)
    w = b[start[a[e]] + within]
    want = b[e] * np.int64(nv) + w
    pos = np.searchsorted(key, want)
    pos[pos == key.size] = 0
    hit = key[pos] == want
    for ids in (a[e][hit], b[e][hit], w[hit]):
        local += np.bincount(ids, minlength=nv).astype(np.uint64)
    return int(hit.sum()), local


def random_multigraph(nv, n, seed):
    """n edges with endpoints uniform in [0, nv): repeated edges, both directions and self-loops."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, nv, n, dtype=np.int64), rng.integers(0, nv, n, dtype=np.int64)
