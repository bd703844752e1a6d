"""CPU oracles of the streaming degrees (gs_deg_*).

(a) ``reference_distribution`` / ``reference_degrees``: the reference's three functions restated
    line by line (example/DegreeDistribution.java EmitVerticesWithChange :73-78, VertexDegreeCounts
    :88-110, DegreeDistributionMap :120-131; SimpleEdgeStream.java DegreeTypeSeparator :451-458,
    DegreeMapFunction :470-477): the record stream, record by record, and both maps.
(b) ``WindowOracle``: the windowed restatement the library follows: per window and vertex the ordered
    composition (A, B) of its steps x -> max(x + a, b), new = max(old + A, B); next to it the plain
    sum old + plus - minus and the at-risk test (the window's deletions at v exceed old).
    ``record`` turns a degree vector into a window's record (degrees, distribution, both deltas,
    stats); tests/degree_streams.py builds its records with it too.
"""
import numpy as np

MASK = (1 << 64) - 1
ALL, OUT, IN = 3, 1, 2                                    # direction masks: bit 0 sources, bit 1 targets


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def pair_mix(v, degree):
    return splitmix64(v ^ splitmix64(degree ^ 0xD1B54A32D192ED03))


def checksum(degrees):
    """degrees: {vertex: degree > 0}"""
    return sum(pair_mix(v, d) for v, d in degrees.items()) & MASK


def _splitmix64_np(x):
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def checksum_arrays(vertices, degrees):
    """checksum() over parallel arrays, vectorised (tests pin it to the scalar form)."""
    v = np.asarray(vertices, dtype=np.uint64)
    d = np.asarray(degrees, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int(_splitmix64_np(v ^ _splitmix64_np(d ^ np.uint64(0xD1B54A32D192ED03))).sum(dtype=np.uint64))


# ---- (a) the reference, record by record ----
class ReferenceDistribution:
    def __init__(self):
        self.verticesWithDegrees = {}
        self.degreesWithCounts = {}

    def event(self, src, dst, add):
        """One edge event; returns the (degree, count) records it prints, in order."""
        out = []
        change = 1 if add else -1
        for vertex in (src, dst):                          # EmitVerticesWithChange
            for t in self._vertex(vertex, change):         # VertexDegreeCounts
                out.append(self._count(t))                 # DegreeDistributionMap
        return out

    def _vertex(self, v, change):
        out = []
        m = self.verticesWithDegrees
        if v in m:
            old = m[v]
            new = old + change
            if new > 0:
                m[v] = new
                out.append((new, 1))
            else:
                del m[v]
            out.append((old, -1))
        elif change > 0:
            m[v] = 1
            out.append((1, 1))
        return out

    def _count(self, t):
        m = self.degreesWithCounts
        if t[0] in m:
            m[t[0]] = m[t[0]] + t[1]
        else:
            m[t[0]] = t[1]
        return (t[0], m[t[0]])

    def distribution(self):
        """count > 0 entries (the reference's map keeps keys whose count fell to 0)"""
        return {d: c for d, c in self.degreesWithCounts.items() if c != 0}


def reference_distribution(events):
    """events: (src, dst, add) triples -> (all records, per-event record lists, final object)"""
    r = ReferenceDistribution()
    per = [r.event(s, d, a) for s, d, a in events]
    return [x for p in per for x in p], per, r


def reference_degrees(edges, collect_in, collect_out):
    """getDegrees (True, True) / getInDegrees (True, False) / getOutDegrees (False, True):
    (vertex, degree) records, per edge."""
    local = {}
    per = []
    for s, t in edges:
        out = []
        keys = ([s] if collect_out else []) + ([t] if collect_in else [])
        for key in keys:
            if key not in local:
                local[key] = 0
            local[key] = local[key] + 1
            out.append((key, local[key]))
        per.append(out)
    return [x for p in per for x in p], per, local


# ---- (b) windows, by composition ----
class WindowOracle:
    def __init__(self, nv, dirs=ALL):
        self.nv = int(nv)
        self.dirs = dirs
        self.deg = np.zeros(self.nv, dtype=np.int64)
        self.risk_windows = 0          # vertex-windows at risk
        self.clamped = 0               # ... whose result differs from the plain sum
        self.risk_unclamped = 0        # ... whose result equals it
        self.vertex_windows = 0
        self.plain_sum_broken = 0      # vertex-windows NOT at risk whose result differs from the plain sum (must stay 0)

    def fold(self, src, dst, add=None):
        """One window. Returns its record: degrees, distribution, both deltas, stats."""
        src = np.asarray(src, dtype=np.int64)
        dst = np.asarray(dst, dtype=np.int64)
        add = np.ones(src.size, dtype=bool) if add is None else np.asarray(add).astype(bool)
        comp = {}                                           # vertex -> [A, B, plus, minus]
        for s, d, a in zip(src.tolist(), dst.tolist(), add.tolist()):
            c = 1 if a else -1
            for e, v in enumerate((s, d)):
                if not (self.dirs >> e) & 1:
                    continue
                x = comp.get(v)
                if x is None:
                    x = comp[v] = [0, 0, 0, 0]
                # (A, B) then the step (c, 0): (A + c, max(B + c, 0))
                x[0], x[1] = x[0] + c, max(x[1] + c, 0)
                x[2 if a else 3] += 1
        before = self.deg.copy()
        for v, (A, B, plus, minus) in comp.items():
            old = int(self.deg[v])
            new = max(old + A, B)
            plain = old + plus - minus
            self.vertex_windows += 1
            if minus > old:
                self.risk_windows += 1
                if new != plain:
                    self.clamped += 1
                else:
                    self.risk_unclamped += 1
            elif new != plain:
                self.plain_sum_broken += 1
            self.deg[v] = new
        return self.record(before)

    def record(self, before=None):
        return record(self.deg, before)


def record(deg, before=None, arrays=False):
    """The record of a degree vector: degrees, distribution, stats and, given the vector before the
    window, both deltas. Pairs of lists, or of numpy arrays when ``arrays`` (large capacities)."""
    deg = np.asarray(deg, dtype=np.int64)
    out = (lambda a, b: (a, b)) if arrays else (lambda a, b: (a.tolist(), b.tolist()))
    vs = np.nonzero(deg)[0]
    dist = np.bincount(deg[vs]) if vs.size else np.zeros(1, dtype=np.int64)
    ds = np.nonzero(dist)[0]
    rec = {"degrees": out(vs, deg[vs]),
           "distribution": out(ds, dist[ds]),
           "stats": {"n_vertices": int(vs.size), "n_degrees": int(ds.size),
                     "max_degree": int(deg.max()) if deg.size else 0,
                     "checksum": checksum_arrays(vs, deg[vs])}}
    if before is not None:
        before = np.asarray(before, dtype=np.int64)
        ch = np.nonzero(deg != before)[0]
        rec["degrees_delta"] = out(ch, deg[ch])
        bvs = np.nonzero(before)[0]
        bdist = np.bincount(before[bvs]) if bvs.size else np.zeros(1, dtype=np.int64)
        m = max(dist.size, bdist.size)
        x = np.zeros(m, dtype=np.int64)
        y = np.zeros(m, dtype=np.int64)
        x[:dist.size] = dist
        y[:bdist.size] = bdist
        x[0] = y[0] = 0
        dk = np.nonzero(x != y)[0]
        rec["distribution_delta"] = out(dk, x[dk])
    return rec


def random_events(nv, n, p_add, seed):
    """A random multigraph event stream, self-loops kept: (src, dst, add)."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, nv, size=n, dtype=np.int64)
    dst = rng.integers(0, nv, size=n, dtype=np.int64)
    if n >= 4:
        dst[n // 3] = src[n // 3]                           # at least one self-loop
    add = rng.random(n) < p_add if p_add < 1.0 else np.ones(n, dtype=bool)
    return src, dst, add
