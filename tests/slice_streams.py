"""Seeded edge-value streams for the neighbourhood-slice tests: (src, dst, values, capacity) with
src / dst / values int64 numpy arrays. The shapes aim at the reduce kernel's seams: it splits the
SORTED entries into tiles of TILE per workgroup and 64 per wave, so what matters is where a row
starts and ends relative to those."""
import numpy as np

WAVE = 64
TILE = 2048                     # entries per workgroup of the reduce kernel (kSliceTile in slice.hip)
ROW_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025)
HUB_EDGES = (1 << 18) + 1       # one row over 129 workgroups of TILE entries (at least 8 are asked for)
assert HUB_EDGES // TILE >= 8

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def values(n, seed):
    """Full-range int64 values: sums wrap, minima and maxima are spread over the sign."""
    return np.random.default_rng(seed).integers(I64_MIN, I64_MAX, size=n, dtype=np.int64, endpoint=True)


def small_values(n, seed):
    return np.random.default_rng(seed).integers(-1000, 1000, size=n, dtype=np.int64)


def uniform(cap, n, seed):
    """Uniform ids in [0, cap), the largest id present."""
    g = np.random.default_rng(seed)
    s = g.integers(0, cap, size=n, dtype=np.int64)
    d = g.integers(0, cap, size=n, dtype=np.int64)
    s[g.integers(0, n)] = cap - 1
    d[g.integers(0, n)] = cap - 1
    return s, d, values(n, seed + 1), cap


def rmat(scale, n, seed, a=0.57, b=0.19, c=0.19):
    """RMAT ids in [0, 2^scale): skewed rows, a few of them long."""
    g = np.random.default_rng(seed)
    s = np.zeros(n, dtype=np.int64)
    d = np.zeros(n, dtype=np.int64)
    for _ in range(scale):
        r = g.random(n)
        s = (s << 1) | (r >= a + b)
        d = (d << 1) | (((r >= a) & (r < a + b)) | (r >= a + b + c))
    return s, d, values(n, seed + 1), 1 << scale


def _interleave(src, dst, val, seed):
    """Arrival order is a seeded shuffle, so it is not the sorted order."""
    p = np.random.default_rng(seed).permutation(src.size)
    return src[p], dst[p], val[p]


def rows_of(lengths, filler, seed):
    """Under "out": a row of `filler` entries at vertex 0 (none when 0), then one row per entry of
    `lengths` at ascending vertices 3, 6, 9, ...; so row k starts at filler + sum(lengths[:k]) of the
    sorted entries. Targets are spread over other ids, which gives "in" and "all" other shapes."""
    keys = [np.zeros(filler, dtype=np.int64)] + [np.full(m, 3 * (k + 1), dtype=np.int64) for k, m in enumerate(lengths)]
    src = np.concatenate(keys)
    cap = 3 * len(lengths) + 3
    g = np.random.default_rng(seed)
    dst = g.integers(0, cap, size=src.size, dtype=np.int64)
    s, d, x = _interleave(src, dst, values(src.size, seed + 1), seed + 2)
    return s, d, x, cap


def row_shapes(filler=0, seed=11):
    return rows_of(ROW_LENGTHS, filler, seed)


def tile_seams(seed=13):
    """Rows that end on, start on and straddle the last lane of a workgroup's tile."""
    lengths = (TILE - 1, 1, 1, TILE - 1, 2, TILE - 2, 1, 2 * TILE + 1, WAVE - 1, 1, WAVE, TILE - WAVE - 1, 1, 1)
    return rows_of(lengths, 0, seed)


def distinct(n, seed=17):
    """n distinct source vertices with one entry each."""
    g = np.random.default_rng(seed)
    src = g.permutation(n).astype(np.int64)
    dst = g.integers(0, n, size=n, dtype=np.int64)
    return src, dst, values(n, seed + 1), n


def hub(n=HUB_EDGES, seed=19):
    """Every edge leaves one vertex: under "out" one row holds every entry."""
    cap = 50000
    g = np.random.default_rng(seed)
    src = np.full(n, 20000, dtype=np.int64)
    dst = g.integers(0, cap, size=n, dtype=np.int64)
    return src, dst, values(n, seed + 1), cap


def hub_and_singles(n=HUB_EDGES, singles=10000, seed=23):
    """The hub plus single-entry vertices with smaller and larger ids than it."""
    cap = 50000
    g = np.random.default_rng(seed)
    others = np.concatenate([np.arange(0, singles // 2), np.arange(20001, 20001 + singles - singles // 2)]).astype(np.int64)
    src = np.concatenate([np.full(n, 20000, dtype=np.int64), others])
    dst = g.integers(0, cap, size=src.size, dtype=np.int64)
    s, d, x = _interleave(src, dst, values(src.size, seed + 1), seed + 2)
    return s, d, x, cap


def two_hubs(n=HUB_EDGES, seed=29):
    """Two hubs with adjacent ids, their entries interleaved."""
    cap = 50000
    g = np.random.default_rng(seed)
    src = 20000 + g.integers(0, 2, size=n, dtype=np.int64)
    dst = g.integers(0, cap, size=n, dtype=np.int64)
    return src, dst, values(n, seed + 1), cap


def value_cases():
    """Small streams over the value edge cases: name -> (src, dst, values, capacity)."""
    a = np.array
    out = {}
    out["extremes"] = (a([1, 1, 2, 2, 3]), a([2, 3, 3, 1, 3]), a([I64_MIN, I64_MAX, I64_MAX, I64_MIN, I64_MIN]), 5)
    out["wrap_up"] = (a([1, 1, 1, 2]), a([2, 2, 3, 1]), a([I64_MAX, I64_MAX, 5, I64_MAX]), 5)
    out["wrap_down"] = (a([1, 1, 1, 2]), a([2, 2, 3, 1]), a([I64_MIN, I64_MIN, -5, I64_MIN]), 5)
    out["all_negative"] = (a([4, 4, 4, 0, 0]), a([0, 1, 2, 4, 4]), a([-7, -3, -9, -1, -2]), 5)
    out["equal"] = (a([2, 2, 2, 3, 3]), a([3, 3, 3, 2, 2]), a([6, 6, 6, 6, 6]), 5)
    out["repeated_edges"] = (a([1, 1, 1, 2, 1]), a([2, 2, 2, 1, 2]), a([30, 10, 20, 5, 15]), 5)
    out["self_loops"] = (a([1, 2, 2, 3, 1]), a([1, 2, 3, 3, 1]), a([4, -8, 16, 32, 64]), 5)
    return {k: (s.astype(np.int64), d.astype(np.int64), x.astype(np.int64), c) for k, (s, d, x, c) in out.items()}


def multi_window(windows=10, window_edges=1000, tail=137, seed=31):
    """A stream of `windows` full windows plus a short last one."""
    n = windows * window_edges + tail
    s, d, x, cap = rmat(10, n, seed)
    return s, d, x, cap, window_edges
