"""Deterministic structured edge streams for the connected-components parity tests (numpy only).

Random graphs (RMAT, Erdos-Renyi) look alike to the fold and close kernels: shallow trees, one
hub-rooted giant from window 1 on, nothing large joining it late, power-of-two capacities whose last
bitmap word is full. The families here are paths, combs, trees and matchings at the capacity
N = 2^20 + 3 (21 id bits: the smallest size at which GSGPU_RING_MIN_BITS=20 selects k_fold_ring; a
3-vertex tail in every bitmap and in the 4-wide parent loads), in windows of W = 2^16 edges (N / 4
edges: the forest is mature after four windows). Every stream is a whole number of windows, padded
with repeats of its own edges. Every generator returns (src, dst) as int64.

  asc_path          edges (i, i+1), i ascending
  desc_path         the same edges, i descending, written (i+1, i): every edge re-roots the chain
  shuffled_path     the path's edges in a seeded permutation: no giant until the last windows
  bitrev_path       the path's edges in bit-reversed order of i
  matching          (2i, 2i+1): N/2 components and never a giant (a young forest throughout), then
                    the windows that chain the pairs by (2i+1, 2i+2) into one path (N/2 edges:
                    nine windows)
  star_max_hub      hub N-1, leaves in permuted order: the root is renamed by every smaller leaf
  binary_tree_desc  vertex N-1-k joined to N-1-(k-1)//2, k ascending
  comb              a shuffled spine, then windows that mix edges inside the giant, teeth, edges
                    between teeth and fresh outside chains; the chains attach late; the root drops
                    64 times at the end (comb() below)
  equal_paths       16 equal paths grown together (no component reaches 25 %), then joined pairwise

odd_capacity_stream(cap): a small stream at an odd capacity with its expected dense labels.

oracle_windows(oracle, name, W) caches the C oracle's per-window checksums and final labels, shared
by every test module of one process.
"""
from __future__ import annotations

import numpy as np

N = (1 << 20) + 3
W = 1 << 16
FAMILIES = ("asc_path", "desc_path", "shuffled_path", "bitrev_path", "matching", "star_max_hub",
            "binary_tree_desc", "comb", "equal_paths")
ODD_CAPS = (1, 2, 3, 31, 33, 1023, 1025, 4097, (1 << 17) + 1, (1 << 21) + 1027)

# comb layout (windows of W edges)
SPINE_LO, SPINE_N = 64, 1 << 18
COMB_SPINE_WINDOWS, COMB_MIX_WINDOWS, COMB_ATTACH_WINDOWS, COMB_DROP_WINDOWS = 4, 8, 2, 2
CHAIN_LEN = 8
# equal_paths layout
EQ_PATHS, EQ_LEN, EQ_LO = 16, 1 << 16, 3
EQ_GROW_WINDOWS, EQ_JOIN_WINDOWS = 16, 4


def _pad(src, dst, rng, window=W):
    """Up to a whole number of windows with repeats of the stream's own edges."""
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    k = (-src.size) % window
    if k:
        i = rng.integers(0, src.size, k)
        src, dst = np.concatenate([src, src[i]]), np.concatenate([dst, dst[i]])
    return src, dst


def _fill(src, dst, k, rng):
    """k repeats of the given edges, either way round."""
    i = rng.integers(0, src.size, k)
    flip = rng.integers(0, 2, k).astype(bool)
    return np.where(flip, dst[i], src[i]), np.where(flip, src[i], dst[i])


def asc_path():
    i = np.arange(N - 1, dtype=np.int64)
    return _pad(i, i + 1, np.random.default_rng(101))


def desc_path():
    i = np.arange(N - 2, -1, -1, dtype=np.int64)
    return _pad(i + 1, i, np.random.default_rng(102))


def shuffled_path():
    rng = np.random.default_rng(103)
    i = rng.permutation(N - 1).astype(np.int64)
    return _pad(i, i + 1, rng)


def bitrev_path():
    bits = 21
    j = np.arange(1 << bits, dtype=np.int64)
    i = np.zeros_like(j)
    for b in range(bits):
        i |= ((j >> b) & 1) << (bits - 1 - b)
    i = i[i < N - 1]
    assert i.size == N - 1
    return _pad(i, i + 1, np.random.default_rng(104))


MATCHING_PAIRS = N // 2


def matching():
    """The matching (padded to whole windows), then the chaining edges."""
    rng = np.random.default_rng(105)
    i = np.arange(MATCHING_PAIRS, dtype=np.int64)
    ms, md = _pad(2 * i, 2 * i + 1, rng)
    cs, cd = _pad(2 * i + 1, 2 * i + 2, rng)
    return np.concatenate([ms, cs]), np.concatenate([md, cd])


def matching_windows():
    """Windows (of W edges) of the matching before the first chaining edge."""
    return -(-MATCHING_PAIRS // W)


def star_max_hub():
    rng = np.random.default_rng(106)
    leaf = rng.permutation(N - 1).astype(np.int64)
    hub = np.full(N - 1, N - 1, dtype=np.int64)
    odd = (np.arange(N - 1) & 1).astype(bool)                 # the hub on either side
    return _pad(np.where(odd, leaf, hub), np.where(odd, hub, leaf), rng)


def binary_tree_desc():
    k = np.arange(1, N, dtype=np.int64)
    return _pad(N - 1 - k, N - 1 - (k - 1) // 2, np.random.default_rng(107))


def comb():
    """Windows 1-4: the shuffled path over the spine [64, 64 + 2^18). Windows 5-12, a quarter each,
    shuffled together: repeated spine edges; teeth (a spine vertex to a fresh leaf; N-1, N-2 and N-3
    are leaves of window 5); edges between leaves of earlier windows (window 5: between spine
    vertices); edges of fresh 8-vertex chains that touch nothing else. Windows 13-14: every outside
    chain attached to the spine by one edge, among repeated member edges. Windows 15-16: repeated
    member edges and, evenly spaced, (63 - k, member) for k = 0..63: the giant's root drops 64 times,
    to 0."""
    rng = np.random.default_rng(108)
    q = W // 4
    sp = SPINE_LO + rng.permutation(SPINE_N - 1).astype(np.int64)
    src, dst = [np.concatenate([sp, sp[:1]])], [np.concatenate([sp + 1, sp[:1] + 1])]
    pool = SPINE_LO + SPINE_N + rng.permutation(N - 3 - SPINE_LO - SPINE_N).astype(np.int64)
    pool = np.concatenate([[N - 1, N - 2, N - 3], pool])      # fresh ids, the tail first
    used = 0
    leaves = np.empty(0, dtype=np.int64)
    nchain = q // (CHAIN_LEN - 1)
    heads = []
    mem_s, mem_d = [sp], [sp + 1]                              # member edges, for the repeats
    for w in range(COMB_MIX_WINDOWS):
        a = SPINE_LO + rng.integers(0, SPINE_N - 1, q)
        ss, sd = a, a + 1                                      # repeated spine edges
        new = pool[used:used + q]; used += q
        at = SPINE_LO + rng.integers(0, SPINE_N, q)
        flip = rng.integers(0, 2, q).astype(bool)
        ts, td = np.where(flip, new, at), np.where(flip, at, new)   # teeth
        if leaves.size:
            ls, ld = leaves[rng.integers(0, leaves.size, q)], leaves[rng.integers(0, leaves.size, q)]
        else:
            ls, ld = SPINE_LO + rng.integers(0, SPINE_N, q), SPINE_LO + rng.integers(0, SPINE_N, q)
        ids = pool[used:used + nchain * CHAIN_LEN].reshape(nchain, CHAIN_LEN); used += nchain * CHAIN_LEN
        cs, cd = ids[:, :-1].ravel(), ids[:, 1:].ravel()
        k = q - cs.size
        cs, cd = np.concatenate([cs, cs[:k]]), np.concatenate([cd, cd[:k]])
        heads.append(ids[np.arange(nchain), rng.integers(0, CHAIN_LEN, nchain)])   # where each is attached later
        s, d = np.concatenate([ss, ts, ls, cs]), np.concatenate([sd, td, ld, cd])
        perm = rng.permutation(W)
        src.append(s[perm]); dst.append(d[perm])
        leaves = np.concatenate([leaves, new])
        mem_s.append(ts); mem_d.append(td)
    assert used <= pool.size
    mem_s, mem_d = np.concatenate(mem_s), np.concatenate(mem_d)
    heads = np.concatenate(heads)
    heads = heads[rng.permutation(heads.size)]
    for part in np.array_split(heads, COMB_ATTACH_WINDOWS):
        at = SPINE_LO + rng.integers(0, SPINE_N, part.size)
        fs, fd = _fill(mem_s, mem_d, W - part.size, rng)
        s, d = np.concatenate([part, fs]), np.concatenate([at, fd])
        perm = rng.permutation(W)
        src.append(s[perm]); dst.append(d[perm])
    per = 64 // COMB_DROP_WINDOWS
    for w in range(COMB_DROP_WINDOWS):
        s, d = _fill(mem_s, mem_d, W, rng)
        pos = (np.arange(per) * (W // per) + W // (2 * per)).astype(np.int64)
        k = w * per + np.arange(per)
        s[pos] = 63 - k
        d[pos] = mem_d[rng.integers(0, mem_d.size, per)]
        src.append(s); dst.append(d)
    return np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64)


def comb_mix_windows():
    return range(COMB_SPINE_WINDOWS, COMB_SPINE_WINDOWS + COMB_MIX_WINDOWS)


def equal_paths():
    """Path p (of 16) runs over the ids 3 + 16 j + p, j < 2^16, so every bitmap word holds vertices
    of all 16. Windows 1-16: their edges shuffled together. Windows 17-20: one joining edge per pair
    (16 -> 8 -> 4 -> 2 -> 1 components) among repeated edges of the paths."""
    rng = np.random.default_rng(109)
    j = np.arange(EQ_LEN - 1, dtype=np.int64)
    a = np.concatenate([EQ_LO + EQ_PATHS * j + p for p in range(EQ_PATHS)])
    perm = rng.permutation(a.size)
    a = a[perm]
    gs, gd = _pad(a, a + EQ_PATHS, rng)
    assert gs.size == EQ_GROW_WINDOWS * W
    src, dst = [gs], [gd]
    comps = [[p] for p in range(EQ_PATHS)]
    for _ in range(EQ_JOIN_WINDOWS):
        s, d = _fill(a, a + EQ_PATHS, W, rng)
        nxt = []
        for i in range(0, len(comps), 2):
            x, y = comps[i], comps[i + 1]
            px, py = x[int(rng.integers(0, len(x)))], y[int(rng.integers(0, len(y)))]
            pos = int(rng.integers(0, W))
            # the later path's vertex first: the hook goes from the larger root to the smaller
            s[pos] = EQ_LO + EQ_PATHS * int(rng.integers(0, EQ_LEN)) + py
            d[pos] = EQ_LO + EQ_PATHS * int(rng.integers(0, EQ_LEN)) + px
            nxt.append(x + y)
        comps = nxt
        src.append(s); dst.append(d)
    return np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64)


_GEN = {"asc_path": asc_path, "desc_path": desc_path, "shuffled_path": shuffled_path, "bitrev_path": bitrev_path,
        "matching": matching, "star_max_hub": star_max_hub, "binary_tree_desc": binary_tree_desc, "comb": comb,
        "equal_paths": equal_paths}
_STREAMS = {}
_ORACLE = {}


def stream(name):
    """(src, dst) of a family: made once per process, read-only."""
    if name not in _STREAMS:
        s, d = _GEN[name]()
        assert s.size == d.size and s.size % W == 0 and s.min() >= 0 and d.min() >= 0 and max(s.max(), d.max()) < N
        s.setflags(write=False); d.setflags(write=False)
        _STREAMS[name] = (s, d)
    return _STREAMS[name]


def oracle_windows(oracle, name, window=W):
    """The C oracle over a family in windows of `window` edges: {"checksums", "counts", "final",
    "final_vertices", "final_components"}; made once per process, read-only."""
    from pyoracle import EMIT_CHECKSUM
    key = (name, window)
    if key not in _ORACLE:
        s, d = stream(name)
        r = oracle.run(s, d, window, partitions=1, threads=1, emit=EMIT_CHECKSUM, label_cap=N, want_final=True)
        r["final"].setflags(write=False)
        _ORACLE[key] = r
    return _ORACLE[key]


def odd_capacity_stream(cap):
    """(src, dst, labels, windows). Caps up to 4097: the whole path over [0, cap) in a seeded order
    (cap 1: the self-loop (0, 0)), in thirds. Larger caps: window 1 a path over the first 5000 ids
    (the giant, root 0), window 2 a path over the last 5000 ids (a component that grows outside the
    giant, up to the last id), window 3 one edge joining the two (every vertex of the second path,
    the one in the last bitmap word included, gets a new label from a close that keeps its giant).
    labels: the expected dense labels (every path vertex its path's minimum, everything else -1);
    windows: the 3 windows [(lo, hi)] the stream is folded in (some are empty at caps 1 to 3)."""
    rng = np.random.default_rng(1000 + cap % 997)
    lab = np.full(cap, -1, dtype=np.int64)
    if cap == 1:
        s = d = np.zeros(1, dtype=np.int64)
        lab[0] = 0
    elif cap <= 4097:
        s = rng.permutation(cap - 1).astype(np.int64)
        d = s + 1
        lab[:] = 0
    if cap <= 4097:
        n = s.size
        cut = [0, (n + 2) // 3, (2 * n + 2) // 3, n]
    else:
        k = 5000
        a = rng.permutation(k - 1).astype(np.int64)
        b = cap - k + rng.permutation(k - 1).astype(np.int64)
        s = np.concatenate([a, b, [cap - k]])
        d = np.concatenate([a + 1, b + 1, [k - 1]])
        lab[:k] = 0
        lab[cap - k:] = 0
        cut = [0, k - 1, 2 * (k - 1), 2 * (k - 1) + 1]
    return s.astype(np.int64), d.astype(np.int64), lab, list(zip(cut[:-1], cut[1:]))
