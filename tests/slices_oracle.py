"""CPU restatements of the neighbourhood slice (SimpleEdgeStream.slice -> SnapshotStream), two that
share no method:

(a) the reference's rule literally: the window's edges become keyed entries through ``reverse()`` /
    ``undirected()``, a dict holds every key's entries in arrival order, and a row is reduced left
    to right with Java ``long`` arithmetic;
(b) numpy: ``np.add.at`` / ``np.minimum.at`` / ``np.maximum.at`` / ``bincount`` over the keyed
    entries, and a stable ``argsort`` for first / last / the CSR rows.

Both emit ordered by vertex (the reference emits in no defined order; its tests compare sorted lines).
"""
import numpy as np

MASK = (1 << 64) - 1
OPS = ("sum", "min", "max", "count", "first", "last")
DIRECTIONS = ("out", "in", "all")


def wrap(x):
    """A Python int as Java long (two's complement, 64 bits)."""
    x &= MASK
    return x - (1 << 64) if x >> 63 else x


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def checksum(records):
    """records: iterable of (vertex, reduced value)"""
    return sum(splitmix64(v ^ splitmix64((x & MASK) ^ 0xD1B54A32D192ED03)) for v, x in records) & MASK


def _splitmix64_np(x):
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def checksum_arrays(vertices, values):
    v = np.asarray(vertices).astype(np.uint64)
    x = np.asarray(values, dtype=np.int64).view(np.uint64)
    with np.errstate(over="ignore"):
        return int(_splitmix64_np(v ^ _splitmix64_np(x ^ np.uint64(0xD1B54A32D192ED03))).sum(dtype=np.uint64))


# ---- (a) the reference, entry by entry ----
def reference_entries(src, dst, val, direction):
    """The keyed entries (key, neighbour, value) of a window in arrival order; val may be None."""
    out = []
    for i in range(len(src)):
        s, d = int(src[i]), int(dst[i])
        x = None if val is None else int(val[i])
        if direction == "out":
            out.append((s, d, x))
        elif direction == "in":
            out.append((d, s, x))                    # reverse()
        else:
            out.append((s, d, x))                    # undirected(): the edge, then its reverse
            out.append((d, s, x))
    return out


def reference_rows(src, dst, val, direction):
    """{vertex: [(neighbour, value), ...] in arrival order}"""
    rows = {}
    for k, nb, x in reference_entries(src, dst, val, direction):
        rows.setdefault(k, []).append((nb, x))
    return rows


_REDUCERS = {
    "sum": lambda a, b: wrap(a + b),
    "min": lambda a, b: a if a <= b else b,
    "max": lambda a, b: a if a >= b else b,
    "first": lambda a, b: a,
    "last": lambda a, b: b,
}


def reference_reduce(rows, op):
    """reduceOnEdges over rows: [(vertex, value)] ordered by vertex; a row of one entry yields its
    value unchanged. "count" is the foldNeighbors counter."""
    out = []
    for k in sorted(rows):
        row = rows[k]
        if op == "count":
            out.append((k, len(row)))
            continue
        f = _REDUCERS[op]
        acc = row[0][1]
        for _, x in row[1:]:
            acc = f(acc, x)
        out.append((k, acc))
    return out


def reference_stats(rows, op):
    rec = reference_reduce(rows, op)
    return {"n_vertices": len(rows), "n_entries": sum(len(r) for r in rows.values()),
            "max_row": max((len(r) for r in rows.values()), default=0), "checksum": checksum(rec)}


def reference_csr(rows):
    """(vertices, offsets, neighbours, values) as lists; values None for a slice without values."""
    v, o, nb, x = [], [0], [], []
    for k in sorted(rows):
        v.append(k)
        nb += [a for a, _ in rows[k]]
        x += [b for _, b in rows[k]]
        o.append(len(nb))
    return v, o, nb, (None if x and x[0] is None else x)


# ---- (b) numpy ----
def numpy_entries(src, dst, val, direction):
    s = np.asarray(src, dtype=np.int64)
    d = np.asarray(dst, dtype=np.int64)
    x = None if val is None else np.asarray(val, dtype=np.int64)
    if direction == "out":
        return s, d, x
    if direction == "in":
        return d, s, x
    key = np.empty(2 * s.size, dtype=np.int64)
    nb = np.empty(2 * s.size, dtype=np.int64)
    key[0::2], key[1::2] = s, d
    nb[0::2], nb[1::2] = d, s
    return key, nb, None if x is None else np.repeat(x, 2)


def numpy_reduce(src, dst, val, direction, op):
    """(vertices, values) ordered by vertex."""
    key, _, x = numpy_entries(src, dst, val, direction)
    if key.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    verts, inv = np.unique(key, return_inverse=True)
    if op == "count":
        return verts, np.bincount(inv, minlength=verts.size).astype(np.int64)
    if op == "sum":
        acc = np.zeros(verts.size, dtype=np.uint64)
        with np.errstate(over="ignore"):
            np.add.at(acc, inv, x.view(np.uint64))
        return verts, acc.view(np.int64)
    if op == "min":
        acc = np.full(verts.size, np.iinfo(np.int64).max, dtype=np.int64)
        np.minimum.at(acc, inv, x)
        return verts, acc
    if op == "max":
        acc = np.full(verts.size, np.iinfo(np.int64).min, dtype=np.int64)
        np.maximum.at(acc, inv, x)
        return verts, acc
    order = np.argsort(key, kind="stable")
    starts = np.nonzero(np.diff(key[order], prepend=key[order][0] - 1))[0]
    if op == "first":
        return verts, x[order[starts]]
    ends = np.append(starts[1:], key.size) - 1
    return verts, x[order[ends]]


def numpy_csr(src, dst, val, direction):
    key, nb, x = numpy_entries(src, dst, val, direction)
    if key.size == 0:
        return np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(0, np.int64), x
    order = np.argsort(key, kind="stable")
    verts, counts = np.unique(key, return_counts=True)
    offs = np.concatenate([[0], np.cumsum(counts)])
    return verts, offs, nb[order], None if x is None else x[order]


def numpy_stats(src, dst, val, direction, op):
    v, r = numpy_reduce(src, dst, val, direction, op)
    _, c = numpy_reduce(src, dst, None, direction, "count")
    return {"n_vertices": int(v.size), "n_entries": int(c.sum()), "max_row": int(c.max()) if c.size else 0,
            "checksum": checksum_arrays(v, r)}
