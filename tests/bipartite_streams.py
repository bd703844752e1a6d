"""Deterministic structured edge streams for the BipartitenessCheck parity tests, and a reference
that shares no code with a union-find (numpy and one scipy call).

Random planted-bipartite multigraphs look alike to csrc/bip.hip: one shallow giant component, at
most one planted same-side edge. The families here build deep trees (paths, cycles closed by an
arbitrary last edge, a chord that arrives before the path it closes), contend for one root word
(star, complete bipartite block) or repeat consistent constraints many times (grid, hypercube), at
the odd capacity NB = 2^18 + 3 in windows of WB = 2^15 edges: the young split sends the first
NB / 4 = 65,536 edges of a handle as one launch (256 waves on one forest), the emission has 65
tiles and the last one holds 3 vertices. `perm` is a seeded label permutation, `shuffle` a seeded
edge order. Every generator takes the size L (a power of two; capacity L + 3, windows of L / 8
edges) so the CPU tests can run it small; streams are not padded, the last window may be short.

  asc_path, desc_path  identity labels, edges (i, i+1) in ascending / descending stream order
  shuffled_path        perm labels, shuffled order
  even_cycle           a cycle of length L + 2 (even) on perm labels, shuffled; one vertex untouched
  odd_cycle            a cycle of length L + 3 (odd), perm, shuffled: only the last window is failed
  odd_cycle_mid        an odd cycle of length L / 4 + 1 whose edges sit at random positions of the
                       first four windows, and a path over the remaining vertices everywhere else
  chord_first          stream edge 0 is (perm[0], perm[L / 2]); the L / 2 path edges between them
                       sit at random positions in [1, 6 windows), the other path edges fill the rest:
                       the odd cycle is closed by a path edge, not by the chord
  matching_loops       L / 2 disjoint pairs on perm labels, each edge three times in both directions,
                       every eighth vertex with a self-loop, the three leftover vertices only as
                       self-loops
  star_max_hub         hub L + 2, every other vertex a leaf, shuffled, the hub on either side
  complete_bipartite   K(m, m), m = sqrt(L), on 2 m perm labels, each edge once, shuffled
  grid                 an m x m lattice, row-major id through perm, shuffled
  grid_diag            grid plus one diagonal (r, c) - (r+1, c+1) as the last edge of window 6
  hypercube            Q_log2(L) at capacity exactly L (a power of two), shuffled, windows of L edges
  rmat_sides           the stream `bench.py --workload bip` times: RMAT at scale log2(L) - 2, edge
                       factor 16, src doubled, dst doubled plus one; capacity L / 2, 16 windows

cover_reference(src, dst, cap): the bipartite double cover. Nodes v and v + cap; a non-loop edge
(a, b) becomes a - b+cap and a+cap - b; a graph is bipartite iff no vertex shares a cover component
with its own copy, and then v's side relative to u is whether v and u (copies 0) share one.
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

L_FULL, L_SMALL, L_TINY = 1 << 18, 1 << 12, 1 << 8
NB = L_FULL + 3
WB = L_FULL // 8
FAMILIES = ("asc_path", "desc_path", "shuffled_path", "even_cycle", "odd_cycle", "odd_cycle_mid", "chord_first",
            "matching_loops", "star_max_hub", "complete_bipartite", "grid", "grid_diag", "hypercube", "rmat_sides")
FAILING = ("odd_cycle", "odd_cycle_mid", "chord_first", "grid_diag")

# src, dst: int64, read-only; cap: vertex capacity; W: window edges; perm: the label permutation
# (None where labels are the identity); info: family-specific facts for the closed forms
Stream = namedtuple("Stream", "src dst cap W perm info")


def _flip(a, b, rng):
    """Every edge either way round."""
    f = rng.integers(0, 2, a.size).astype(bool)
    return np.where(f, b, a), np.where(f, a, b)


def _shuffle(a, b, rng):
    o = rng.permutation(a.size)
    return a[o], b[o]


def _scatter(n, first_a, first_b, positions, rest_a, rest_b):
    """A stream of n edges: the `first` edges at `positions`, the `rest` edges, in their order, at
    the remaining positions."""
    assert first_a.size == positions.size and first_a.size + rest_a.size == n
    a = np.empty(n, dtype=np.int64)
    b = np.empty(n, dtype=np.int64)
    free = np.ones(n, dtype=bool)
    free[positions] = False
    assert int(free.sum()) == rest_a.size
    a[positions], b[positions] = first_a, first_b
    a[free], b[free] = rest_a, rest_b
    return a, b


def asc_path(L):
    i = np.arange(L + 2, dtype=np.int64)
    return Stream(i, i + 1, L + 3, L // 8, None, {})


def desc_path(L):
    i = np.arange(L + 1, -1, -1, dtype=np.int64)
    return Stream(i, i + 1, L + 3, L // 8, None, {})


def shuffled_path(L):
    rng = np.random.default_rng(201)
    nb = L + 3
    perm = rng.permutation(nb).astype(np.int64)
    i = rng.permutation(nb - 1)
    a, b = _flip(perm[i], perm[i + 1], rng)
    return Stream(a, b, nb, L // 8, perm, {})


def _cycle(L, length, seed):
    rng = np.random.default_rng(seed)
    nb = L + 3
    perm = rng.permutation(nb).astype(np.int64)
    i = np.arange(length)
    a, b = _flip(perm[i], perm[(i + 1) % length], rng)
    a, b = _shuffle(a, b, rng)
    return Stream(a, b, nb, L // 8, perm, {"length": length})


def even_cycle(L):
    return _cycle(L, L + 2, 202)


def odd_cycle(L):
    return _cycle(L, L + 3, 203)


def odd_cycle_mid(L):
    rng = np.random.default_rng(204)
    nb, wb, C = L + 3, L // 8, L // 4 + 1
    perm = rng.permutation(nb).astype(np.int64)
    i = np.arange(C)
    ca, cb = _flip(perm[i], perm[(i + 1) % C], rng)
    j = C + rng.permutation(nb - C - 1)
    pa, pb = _flip(perm[j], perm[j + 1], rng)
    pos = rng.choice(4 * wb, C, replace=False)
    a, b = _scatter(nb - 1, ca, cb, pos, pa, pb)
    return Stream(a, b, nb, wb, perm, {"length": C})


def chord_first(L):
    rng = np.random.default_rng(205)
    nb, wb, H = L + 3, L // 8, L // 2
    perm = rng.permutation(nb).astype(np.int64)
    i = rng.permutation(H)                                         # the segment perm[0] .. perm[H]
    sa, sb = _flip(perm[i], perm[i + 1], rng)
    j = H + rng.permutation(nb - 1 - H)
    ra, rb = _flip(perm[j], perm[j + 1], rng)
    pos = 1 + rng.choice(6 * wb - 1, H, replace=False)
    a, b = _scatter(nb, np.concatenate([perm[:1], sa]), np.concatenate([perm[H:H + 1], sb]),
                    np.concatenate([[0], pos]), ra, rb)
    return Stream(a, b, nb, wb, perm, {"length": H + 1})


def matching_loops(L):
    rng = np.random.default_rng(206)
    nb = L + 3
    perm = rng.permutation(nb).astype(np.int64)
    x, y = perm[0:L:2], perm[1:L:2]
    loops = np.concatenate([perm[0:L:8], perm[L:]])
    a = np.concatenate([x, y, x, loops])
    b = np.concatenate([y, x, y, loops])
    a, b = _shuffle(a, b, rng)
    return Stream(a, b, nb, L // 8, perm, {"components": L // 2 + 3})


def star_max_hub(L):
    rng = np.random.default_rng(207)
    nb = L + 3
    leaf = rng.permutation(nb - 1).astype(np.int64)
    hub = np.full(nb - 1, nb - 1, dtype=np.int64)
    a, b = _flip(leaf, hub, rng)
    return Stream(a, b, nb, L // 8, None, {})


def _side(L):
    m = int(round(L ** 0.5))
    assert m * m == L
    return m


def complete_bipartite(L):
    rng = np.random.default_rng(208)
    nb, m = L + 3, _side(L)
    perm = rng.permutation(nb).astype(np.int64)
    left, right = perm[:m], perm[m:2 * m]
    a, b = _flip(np.repeat(left, m), np.tile(right, m), rng)
    a, b = _shuffle(a, b, rng)
    return Stream(a, b, nb, L // 8, perm, {"m": m})


def _grid_edges(L, rng):
    m = _side(L)
    perm = rng.permutation(L + 3).astype(np.int64)
    idx = np.arange(L, dtype=np.int64).reshape(m, m)
    u = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    v = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    a, b = _flip(perm[u], perm[v], rng)
    a, b = _shuffle(a, b, rng)
    return a, b, perm, m


def grid(L):
    a, b, perm, m = _grid_edges(L, np.random.default_rng(209))
    return Stream(a, b, L + 3, L // 8, perm, {"m": m})


def grid_diag(L):
    rng = np.random.default_rng(209)                               # grid's stream, plus the diagonal
    a, b, perm, m = _grid_edges(L, rng)
    wb = L // 8
    r, c = (int(x) for x in rng.integers(0, m - 1, 2))
    at = 6 * wb - 1
    a = np.insert(a, at, perm[r * m + c])
    b = np.insert(b, at, perm[(r + 1) * m + c + 1])
    return Stream(a, b, L + 3, wb, perm, {"m": m, "diag_at": at})


def hypercube_edges(L):
    """Every edge of Q_log2(L) once, (v, v | bit) with the bit clear in v, bit by bit."""
    k = L.bit_length() - 1
    assert 1 << k == L
    v = np.arange(L, dtype=np.int64)
    a = np.concatenate([v[(v >> bit) & 1 == 0] for bit in range(k)])
    b = np.concatenate([v[(v >> bit) & 1 == 0] | (1 << bit) for bit in range(k)])
    return a, b


def hypercube(L):
    rng = np.random.default_rng(210)
    a, b = hypercube_edges(L)
    a, b = _flip(a, b, rng)
    a, b = _shuffle(a, b, rng)
    return Stream(a, b, L, L, None, {})


def hypercube_sign(L):
    """Closed form of Q_log2(L): key 0, a vertex is on 0's side iff its popcount is even."""
    v = np.arange(L, dtype=np.int64)
    pop = np.zeros(L, dtype=np.int64)
    for bit in range(L.bit_length() - 1):
        pop += (v >> bit) & 1
    return pop % 2 == 0


@functools.lru_cache(maxsize=None)
def staging_stream():
    """2^22 + 5 edges for the host staging loop (chunks of 2^22 edges): Q18's edge list taken
    twice, reshuffled and cut to that length."""
    rng = np.random.default_rng(211)
    a, b = hypercube_edges(L_FULL)
    a, b = _flip(np.concatenate([a, a]), np.concatenate([b, b]), rng)
    a, b = _shuffle(a, b, rng)
    n = (1 << 22) + 5
    a, b = np.ascontiguousarray(a[:n]), np.ascontiguousarray(b[:n])
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


RMAT_SEED, RMAT_EDGE_FACTOR = 1, 16


def rmat_sides(L):
    from pyoracle import coracle
    scale = L.bit_length() - 3
    n = RMAT_EDGE_FACTOR << scale
    s, d = coracle().gen_rmat(0, n, scale, RMAT_SEED)
    return Stream(2 * s, 2 * d + 1, 2 << scale, n // 16, None, {"scale": scale})


_GEN = {"asc_path": asc_path, "desc_path": desc_path, "shuffled_path": shuffled_path, "even_cycle": even_cycle,
        "odd_cycle": odd_cycle, "odd_cycle_mid": odd_cycle_mid, "chord_first": chord_first,
        "matching_loops": matching_loops, "star_max_hub": star_max_hub, "complete_bipartite": complete_bipartite,
        "grid": grid, "grid_diag": grid_diag, "hypercube": hypercube, "rmat_sides": rmat_sides}


@functools.lru_cache(maxsize=None)
def stream(name, L=L_FULL):
    """The family at size L: made once per process, read-only."""
    st = _GEN[name](L)
    a = np.ascontiguousarray(st.src, dtype=np.int64)
    b = np.ascontiguousarray(st.dst, dtype=np.int64)
    assert a.size == b.size and a.min() >= 0 and b.min() >= 0 and max(a.max(), b.max()) < st.cap
    a.setflags(write=False)
    b.setflags(write=False)
    if st.perm is not None:
        st.perm.setflags(write=False)
    return st._replace(src=a, dst=b)


def n_windows(name, L=L_FULL):
    st = stream(name, L)
    return -(-st.src.size // st.W)


# ---- the reference ----
def cover_reference(src, dst, cap):
    """(ok, vertices, keys, signs) of the graph so far: ok iff it is bipartite; then every seen
    vertex in ascending order, the minimum seen vertex of its component, and whether it is on that
    vertex's side. A failed state has no entries (the reference's "(false,{})")."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    s = np.asarray(src, dtype=np.int64)
    d = np.asarray(dst, dtype=np.int64)
    seen = np.zeros(cap, dtype=bool)
    seen[s] = True
    seen[d] = True
    m = s != d                                                     # self-loops only mark their vertex
    a, b = s[m], d[m]
    rows = np.concatenate([a, a + cap])
    cols = np.concatenate([b + cap, b])
    g = coo_matrix((np.ones(rows.size, dtype=np.int8), (rows, cols)), shape=(2 * cap, 2 * cap))
    _, lab = connected_components(g, directed=False)
    lo, hi = lab[:cap], lab[cap:]
    v = np.nonzero(seen)[0].astype(np.int64)
    if np.any(lo[v] == hi[v]):
        e = np.empty(0, dtype=np.int64)
        return False, e, e.copy(), np.empty(0, dtype=bool)
    comp = np.minimum(lo, hi)[v]                                   # names the pair of cover components
    _, first, inv = np.unique(comp, return_index=True, return_inverse=True)
    keys = v[first][inv]                                           # v ascends: first = the minimum
    signs = lo[v] == lo[keys]
    return True, v, keys, signs


def checksum(vertices, keys, signs):
    """gs_bip_checksum's sum over (v, key << 1 | sign) (test_gpu_bipartite._checksum, vectorised)."""
    from pyoracle import _np_splitmix64
    v = np.asarray(vertices).astype(np.uint64)
    lab = (np.asarray(keys).astype(np.uint64) << np.uint64(1)) | np.asarray(signs).astype(np.uint64)
    mix = _np_splitmix64(v ^ _np_splitmix64(lab ^ np.uint64(0xD1B54A32D192ED03)))
    with np.errstate(over="ignore"):
        return int(np.sum(mix, dtype=np.uint64))


class Ref:
    """One reference state, stored densely (4 + 1 bytes per id); ok False: no entries."""

    def __init__(self, ok, vertices, keys, signs, cap):
        self.ok = bool(ok)
        self.n_vertices = int(vertices.size)
        self.n_components = int(np.count_nonzero(vertices == keys))
        self.checksum = checksum(vertices, keys, signs)
        self._key = np.full(cap, -1, dtype=np.int32)
        self._key[vertices] = keys
        self._sign = np.zeros(cap, dtype=bool)
        self._sign[vertices] = signs
        self._key.setflags(write=False)
        self._sign.setflags(write=False)

    @property
    def status(self):
        return self.ok, self.n_vertices, self.n_components

    def pairs(self):
        v = np.nonzero(self._key >= 0)[0].astype(np.int64)
        return v, self._key[v].astype(np.int64), self._sign[v]

    def string(self):
        """The reference's toString (tiny cases only)."""
        if not self.ok:
            return "(false,{})"
        comps = {}
        for v, k, s in zip(*(x.tolist() for x in self.pairs())):
            comps.setdefault(k, []).append("%d=(%d,%s)" % (v, v, "true" if s else "false"))
        return "(true,{%s})" % ", ".join("%d={%s}" % (k, ", ".join(m)) for k, m in sorted(comps.items()))


@functools.lru_cache(maxsize=None)
def reference_prefix(name, n, L=L_FULL):
    """The reference after the family's first n edges."""
    st = stream(name, L)
    return Ref(*cover_reference(st.src[:n], st.dst[:n], st.cap), st.cap)


@functools.lru_cache(maxsize=None)
def reference_windows(name, W=None, L=L_FULL):
    """The reference after every window of W edges (default: the family's own), as a tuple of Ref."""
    st = stream(name, L)
    W = W or st.W
    return tuple(reference_prefix(name, min(hi, st.src.size), L) for hi in range(W, st.src.size + W, W))


def first_failed_window(name, L=L_FULL):
    """Index of the first failed window, or None."""
    for w, r in enumerate(reference_windows(name, None, L)):
        if not r.ok:
            return w
    return None
