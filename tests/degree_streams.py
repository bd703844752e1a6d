"""Seeded structured event streams for the streaming degrees (gs_deg_*) and a vectorised fold of
the windowed composition, for sizes at which WindowOracle's per-event loop is too slow.

``fold_vec`` restates a window as prefix sums: the steps x -> max(x + c, 0), c = +-1, of one vertex
in stream order, with prefix sums S_1..S_n of the c, end at S_n + max(old, -min(0, min_j S_j)) (the
clamp is the reflection of the walk old + S_j at 0). deg.hip composes (a, b) pairs in a segmented
scan or sums counters; neither forms a prefix minimum.

Each family reaches a region of deg.hip that needs a size the random streams never have:

* ``wide_events``    21 vertex bits, an odd capacity whose last bitmap word is partial and holds an
                     at-risk vertex, 2.6 M events (a second trip of every grid-stride loop and of
                     k_deg_count's tile loop), more than 2^19 touched vertices;
* ``hub_ladder``     the default dense cut: degrees 1,023 / 1,024 (the LDS cut), 65,535 / 65,536 (the
                     dense / sparse cut) and beyond, the maximum's rescan, runs of 70,000 and of
                     200,000 steps at one vertex with clamps inside and at the end;
* ``two_long_runs``  two runs of 150,000+ steps whose keys alternate in the input."""
import functools

import numpy as np

from degrees_oracle import ALL, IN, OUT, record

WIDE_CAPACITY = (1 << 20) + 3
GRID_SPAN = 2048 * 256             # deg.hip kDegMaxBlocks x kDegThreads: items of one grid-stride trip
COUNT_SPAN = 2048 * 1024           # events one trip of k_deg_count's tile loop covers
LDS_DEG = 1024                     # deg.hip kLdsDeg
DENSE = 1 << 16                    # deg.hip kDegDefaultDense


class Fold:
    """What fold_vec reports next to the new degree vector."""
    __slots__ = ("deg", "touched", "risk", "clamped", "longest_run")


def fold_vec(deg, src, dst, add=None, dirs=ALL):
    """One window over the degree vector ``deg`` (not changed); returns a Fold whose ``deg`` is the
    new vector, ``touched`` the window's vertices, ``risk`` / ``clamped`` masks over them (the
    window's deletions exceed the old degree / the result differs from the plain sum)."""
    deg = np.asarray(deg, dtype=np.int64)
    src = np.asarray(src, dtype=np.int64)
    dst = np.asarray(dst, dtype=np.int64)
    n = src.size
    change = np.ones(n, dtype=np.int64) if add is None else np.where(np.asarray(add).astype(bool), 1, -1).astype(np.int64)
    if dirs == ALL:                                        # vertex events in stream order: position 2 i + end
        v = np.stack([src, dst], axis=1).ravel()
        c = np.repeat(change, 2)
    else:
        v, c = (src if dirs == OUT else dst), change
    out = Fold()
    out.deg = deg.copy()
    if v.size == 0:
        out.touched = np.empty(0, dtype=np.int64)
        out.risk = out.clamped = np.empty(0, dtype=bool)
        out.longest_run = 0
        return out
    order = np.argsort(v, kind="stable")                   # by (vertex, position)
    v, c = v[order], c[order]
    start = np.flatnonzero(np.concatenate([[True], v[1:] != v[:-1]]))
    end = np.concatenate([start[1:], [v.size]]) - 1
    run = np.cumsum(c)
    base = run[start] - c[start]                           # the running sum before the vertex's first step
    s_n = run[end] - base
    s_min = np.minimum.reduceat(run, start) - base
    vs = v[start]
    old = deg[vs]
    new = s_n + np.maximum(old, -np.minimum(0, s_min))
    minus = np.add.reduceat((c < 0).astype(np.int64), start)
    out.deg[vs] = new
    out.touched = vs
    out.risk = minus > old
    out.clamped = new != old + s_n
    out.longest_run = int((end - start + 1).max())
    return out


def fold_records(capacity, windows, dirs=ALL):
    """Fold ``windows`` = [(src, dst, add or None)] from an empty summary. Returns (records, folds):
    per window the record (numpy arrays) of degrees_oracle.record and fold_vec's report."""
    deg = np.zeros(capacity, dtype=np.int64)
    recs, folds = [], []
    for src, dst, add in windows:
        f = fold_vec(deg, src, dst, add, dirs)
        recs.append(record(f.deg, deg, arrays=True))
        folds.append(f)
        deg = f.deg
    return tuple(recs), tuple(folds)


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def cut(src, dst, add, W):
    return [(src[lo:lo + W], dst[lo:lo + W], None if add is None else add[lo:lo + W]) for lo in range(0, src.size, W)]


# ---- wide_events ----
WIDE_N = (1 << 21) + (1 << 19) + 77
WIDE_WINDOW = 1 << 19
WIDE_RUN_AT = (0, (1 << 20) + 100)      # where the clamping runs of vertex 0 and vertex capacity - 1 begin
WIDE_RUN = (40, 10)                     # deletions, then additions


@functools.lru_cache(maxsize=None)
def wide_events(seed=30):
    """2^21 + 2^19 + 77 random events over [0, 2^20 + 3), p_add = 0.6. Vertex 0 (from event 0) and
    vertex capacity - 1 (from event 2^20 + 100) each get a run of 40 deletions and then 10
    additions as a source. Returns (src, dst, add, capacity)."""
    rng = np.random.default_rng(seed)
    cap, n = WIDE_CAPACITY, WIDE_N
    src = rng.integers(0, cap, size=n, dtype=np.int64)
    dst = rng.integers(0, cap, size=n, dtype=np.int64)
    add = rng.random(n) < 0.6
    for v, at in zip((0, cap - 1), WIDE_RUN_AT):
        k = sum(WIDE_RUN)
        src[at:at + k] = v
        add[at:at + WIDE_RUN[0]] = False
        add[at + WIDE_RUN[0]:at + k] = True
    _frozen(src, dst, add)
    return src, dst, add, cap


@functools.lru_cache(maxsize=None)
def wide_events_reference(windowed):
    src, dst, add, cap = wide_events()
    return fold_records(cap, cut(src, dst, add, WIDE_WINDOW if windowed else src.size))


# ---- hub_ladder ----
LADDER_CAPACITY = (1 << 18) + 5
LADDER_HUB, LADDER_HUB2 = 77777, 5
LADDER_DEGREES = (1023, 1024, 65535, 65536, 135536, 135536, 65535, 1000, 0)   # the first hub after windows 0..8
LADDER_LAST = 200000


@functools.lru_cache(maxsize=None)
def hub_ladder(seed=31):
    """Windows [(src, dst, add or None)] over capacity 2^18 + 5, hubs as sources and targets in turn,
    leaves spread over the ids up to capacity - 1 (the first leaf). Additions-only windows carry no
    event array. Returns (windows, capacity)."""
    rng = np.random.default_rng(seed)
    cap, hub, hub2 = LADDER_CAPACITY, LADDER_HUB, LADDER_HUB2
    others = np.setdiff1d(np.arange(cap - 1, dtype=np.int64), [hub, hub2])
    leaves = np.concatenate([[cap - 1], rng.permutation(others)])

    def star(h, lo, hi, adding):
        """the edges h - leaves[lo:hi], every other one given leaf -> hub; deletions in reverse order"""
        lv = leaves[lo:hi] if adding else leaves[lo:hi][::-1]
        hh = np.full(lv.size, h, dtype=np.int64)
        flip = (np.arange(lv.size) % 2).astype(bool)
        return np.where(flip, lv, hh), np.where(flip, hh, lv), None if adding else np.zeros(lv.size, dtype=bool)

    windows = [star(hub, 0, 1023, True), star(hub, 1023, 1024, True), star(hub, 1024, 65535, True),
               star(hub, 65535, 65536, True), star(hub, 65536, 135536, True),
               star(hub2, 0, 40000, True),
               star(hub, 65535, 135536, False), star(hub, 1000, 65535, False),
               star(hub, 0, 1001, False)]                  # one deletion more than the hub's degree
    # the first hub alone: blocks of additions and deletions; the running degree reaches 0 after
    # blocks 2 (10 steps clamp), 4 (exactly 0), 8 (3 clamp) and at the end (7 clamp)
    blocks = [30000, -30010, 40000, -40000, 20000, -10000, 5000, -15003, 4990, -4997]
    assert sum(abs(b) for b in blocks) == LADDER_LAST
    add = np.concatenate([np.full(abs(b), b > 0) for b in blocks])
    lv = leaves[rng.integers(0, leaves.size, size=LADDER_LAST)]
    hh = np.full(LADDER_LAST, hub, dtype=np.int64)
    flip = rng.random(LADDER_LAST) < 0.5
    windows.append((np.where(flip, lv, hh), np.where(flip, hh, lv), add))
    for w in windows:
        _frozen(*w)
    return tuple(windows), cap


@functools.lru_cache(maxsize=None)
def hub_ladder_reference():
    windows, cap = hub_ladder()
    return fold_records(cap, windows)


# ---- two_long_runs ----
TWO_CAPACITY = 70001                    # 70,001 = 2,187 x 32 + 17: the last bitmap word is partial
TWO_U, TWO_W = TWO_CAPACITY - 1, 33
TWO_WINDOWS = (300000, 100001)


@functools.lru_cache(maxsize=None)
def two_long_runs(direction, seed=32):
    """Events whose sources alternate between two vertices, p_add = 0.5 (each degree is a walk
    reflected at 0). direction "out": targets are random other vertices; "all": the target is the
    other one of the two, so each takes every vertex event in turn. Returns (windows, capacity, dirs)."""
    rng = np.random.default_rng(seed)
    n = sum(TWO_WINDOWS)
    even = np.arange(n) % 2 == 0
    src = np.where(even, TWO_U, TWO_W).astype(np.int64)
    if direction == "all":
        dst = np.where(even, TWO_W, TWO_U).astype(np.int64)
    else:
        dst = rng.integers(100, TWO_CAPACITY - 100, size=n, dtype=np.int64)
    add = rng.random(n) < 0.5
    _frozen(src, dst, add)
    k = TWO_WINDOWS[0]
    return ((src[:k], dst[:k], add[:k]), (src[k:], dst[k:], add[k:])), TWO_CAPACITY, {"all": ALL, "out": OUT, "in": IN}[direction]


@functools.lru_cache(maxsize=None)
def two_long_runs_reference(direction):
    windows, cap, dirs = two_long_runs(direction)
    return fold_records(cap, windows, dirs)
