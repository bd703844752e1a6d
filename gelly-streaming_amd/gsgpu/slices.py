"""Neighbourhood slices on the device (include/gsgpu.h gs_slice_*): Python mirror of the reference's
``SimpleEdgeStream.slice(size, direction)`` -> ``SnapshotStream`` (SimpleEdgeStream.java:135-167)
with ``reduceOnEdges`` / ``foldNeighbors`` / ``applyOnNeighbors`` (SnapshotStream.java:61-131).

A count window of edges ``(s, d, x)``, ``x`` an int64 edge value, becomes entries ``(key, neighbour,
value)``: ``"out"`` ``(s, d, x)``, ``"in"`` ``(d, s, x)``, ``"all"`` both, ``(s, d, x)`` first. The
row of a vertex is its entries in arrival order; ``reduce_on_edges`` reduces every row's values left
to right and ``rows`` emits the rows as CSR, which is what ``apply_on_neighbors`` and
``fold_neighbors`` run a host function over. Records are ordered by vertex.
"""
from __future__ import annotations

import ctypes
from typing import Callable, List, Optional, Tuple

import numpy as np

from . import _abi
from ._abi import GsSliceWindowStats, call
from .summary import _as_torch_stream, _buf, _current_raw_stream, _first_cuda_tensor, _is_torch, _stream_ptr

U64 = ctypes.c_uint64
_DIRS = {"out": _abi.GS_SLICE_OUT, "in": _abi.GS_SLICE_IN, "all": _abi.GS_SLICE_ALL}
OPS = {"sum": _abi.GS_SLICE_SUM, "min": _abi.GS_SLICE_MIN, "max": _abi.GS_SLICE_MAX, "count": _abi.GS_SLICE_COUNT,
       "first": _abi.GS_SLICE_FIRST, "last": _abi.GS_SLICE_LAST}
_STATS_DTYPE = np.dtype([("n_vertices", np.uint64), ("n_entries", np.uint64), ("max_row", np.uint64),
                         ("checksum", np.uint64)])


def _op(op) -> int:
    if isinstance(op, str):
        if op not in OPS:
            raise ValueError("op must be one of %s" % ", ".join(sorted(OPS)))
        return OPS[op]
    return int(op)


def _values(values, n: int):
    """(pointer, keepalive) of a nullable int64 edge-value array."""
    if values is None:
        return None, None
    if _is_torch(values):
        import torch
        if values.dtype != torch.int64 or not values.is_contiguous():
            raise TypeError("values: a contiguous int64 tensor is expected")
        if values.numel() != n:
            raise ValueError("values: %d entries for %d edges" % (values.numel(), n))
        return ctypes.c_void_p(values.data_ptr()), values
    a = np.ascontiguousarray(np.asarray(values).astype(np.int64, copy=False))
    if a.size != n:
        raise ValueError("values: %d entries for %d edges" % (a.size, n))
    return a.ctypes.data_as(ctypes.c_void_p), a


def _out_ptr(x):
    return ctypes.c_void_p(x.data_ptr()) if _is_torch(x) else x.ctypes.data_as(ctypes.c_void_p)


class SnapshotStream:
    """The slice of one window at a time; dense ids in [0, vertex_capacity), capacity <= 2^32.

    ``direction``: "out" (rows of sources, the default), "in" (rows of targets) or "all" (both ends
    of every edge)."""

    def __init__(self, vertex_capacity: int, direction: str = "out", id_bits: int = 64, device: int = 0, stream=None):
        if direction not in _DIRS:
            raise ValueError("direction must be 'out', 'in' or 'all'")
        self.capacity = int(vertex_capacity)
        self.id_bits = int(id_bits)
        self.direction = direction
        self._h = None
        h = ctypes.c_void_p()
        call("gs_slice_create", ctypes.byref(h), self.capacity, self.id_bits, int(device), _DIRS[direction])
        self._h = h
        self._hs: Optional[int] = None
        self._n = 0                                   # edges of the slice held
        self._has_values = False
        if stream is not None:
            self.set_stream(stream)

    @property
    def handle(self) -> ctypes.c_void_p:
        if self._h is None:
            raise RuntimeError("SnapshotStream is closed")
        return self._h

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            _abi.lib().gs_slice_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - GC timing
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self) -> "SnapshotStream":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def set_stream(self, stream) -> None:
        call("gs_slice_set_stream", self.handle, _stream_ptr(stream))
        self._hs = None

    def _stream(self) -> int:
        if self._hs is None:
            s = ctypes.c_void_p()
            call("gs_slice_get_stream", self.handle, ctypes.byref(s))
            self._hs = int(s.value or 0)
        return self._hs

    def _after_torch(self, *objs) -> None:
        """Device tensors a call reads were produced in torch's stream order: the handle's stream
        waits for torch's current stream first (an event, no host wait), as TriangleCounter does.
        Every call here ends with a host wait on the handle's stream, so nothing is owed back."""
        t = _first_cuda_tensor(objs)
        if t is None:
            return
        hs = self._stream()
        if hs == _current_raw_stream(t):
            return
        import torch
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(t.device))
        _as_torch_stream(hs, t.device).wait_event(ev)

    def sync(self) -> None:
        call("gs_slice_sync", self.handle)

    def _vdtype(self):
        return np.uint32 if self.id_bits == 32 else np.int64

    def _entries(self, n: int) -> int:
        return 2 * n if self.direction == "all" else n

    def _edges(self, src, dst, values):
        ps, ks, n = _buf(src, self.id_bits, "src")
        pd, kd, m = _buf(dst, self.id_bits, "dst")
        if n != m:
            raise ValueError("src and dst lengths differ (%d, %d)" % (n, m))
        pv, kv = _values(values, n)
        self._after_torch(ks, kd, kv)
        return ps, pd, pv, n, (ks, kd, kv)

    # ---- one window ----
    def window(self, src, dst, values=None) -> "SnapshotStream":
        """Build the slice of these edges; it replaces the one held. ``values=None``: a slice
        without edge values, on which only "count" and ``rows`` (without values) apply."""
        ps, pd, pv, n, keep = self._edges(src, dst, values)
        call("gs_slice_window", self.handle, ps, pd, pv, n)
        del keep
        self._n = n
        self._has_values = values is not None
        return self

    def reduce_on_edges(self, op, out=None):
        """reduceOnEdges: ``(vertices, values)``, one record per row, ordered by vertex. ``out``: a
        pair of arrays or device tensors to write into; the number of records is returned then."""
        code = _op(op)
        if out is not None:
            v, x = out
            self._after_torch(v, x)
            n = U64()
            call("gs_slice_reduce", self.handle, code, _out_ptr(v), _out_ptr(x), min(len(v), len(x)), ctypes.byref(n))
            return int(n.value)
        cap = max(min(self._entries(self._n), self.capacity), 1)
        while True:
            v = np.empty(cap, dtype=self._vdtype())
            x = np.empty(cap, dtype=np.int64)
            n = U64()
            rc = _abi.lib().gs_slice_reduce(self.handle, code, _out_ptr(v), _out_ptr(x), cap, ctypes.byref(n))
            if rc == _abi.GS_ERR_CAPACITY and int(n.value) > cap:      # (the size kept here is only a first guess)
                cap = int(n.value)
                continue
            if rc != _abi.GS_OK:
                msg = _abi.lib().gs_last_error()
                raise _abi.GsError(rc, "gs_slice_reduce", msg.decode() if msg else "")
            return v[:int(n.value)], x[:int(n.value)]

    def rows(self, out=None):
        """The slice as CSR: ``(vertices, offsets, neighbours, values)``; row r is
        ``offsets[r]:offsets[r + 1]`` of neighbours and values, in arrival order. ``values`` is None
        for a slice without values. ``out``: four arrays or device tensors to write into (values may
        be None); ``(n_vertices, n_entries)`` is returned then."""
        nv, ne = U64(), U64()
        if out is not None:
            v, o, nb, x = out
            self._after_torch(v, o, nb, x)
            call("gs_slice_rows", self.handle, _out_ptr(v), _out_ptr(o), _out_ptr(nb), None if x is None else _out_ptr(x),
                 min(len(v), len(o) - 1), len(nb) if x is None else min(len(nb), len(x)), ctypes.byref(nv), ctypes.byref(ne))
            return int(nv.value), int(ne.value)
        ecap = max(self._entries(self._n), 1)
        vcap = max(min(ecap, self.capacity), 1)
        while True:
            v = np.empty(vcap, dtype=self._vdtype())
            o = np.zeros(vcap + 1, dtype=np.uint64)
            nb = np.empty(ecap, dtype=self._vdtype())
            x = np.empty(ecap, dtype=np.int64) if self._has_values else None
            rc = _abi.lib().gs_slice_rows(self.handle, _out_ptr(v), _out_ptr(o), _out_ptr(nb), None if x is None else _out_ptr(x),
                                          vcap, ecap, ctypes.byref(nv), ctypes.byref(ne))
            a, e = int(nv.value), int(ne.value)
            if rc == _abi.GS_ERR_CAPACITY and (a > vcap or e > ecap):  # (the sizes kept here are only a first guess)
                vcap, ecap = max(a, vcap), max(e, ecap)
                continue
            if rc != _abi.GS_OK:
                msg = _abi.lib().gs_last_error()
                raise _abi.GsError(rc, "gs_slice_rows", msg.decode() if msg else "")
            return v[:a], o[:a + 1], nb[:e], None if x is None else x[:e]

    def apply_on_neighbors(self, fn: Callable) -> list:
        """applyOnNeighbors: ``fn(vertex, neighbours, values)`` per row, in vertex order, on the host;
        what it returns is collected (None is dropped, as a function that collects nothing)."""
        v, o, nb, x = self.rows()
        res = []
        for r in range(len(v)):
            a, b = int(o[r]), int(o[r + 1])
            got = fn(int(v[r]), nb[a:b], None if x is None else x[a:b])
            if got is not None:
                res.append(got)
        return res

    def fold_neighbors(self, initial, fn: Callable) -> List[Tuple[int, object]]:
        """foldNeighbors: per row ``acc = fn(acc, vertex, neighbour, value)`` entry by entry in
        arrival order, from ``initial``; one ``(vertex, acc)`` per row."""
        v, o, nb, x = self.rows()
        res = []
        for r in range(len(v)):
            acc = initial
            for j in range(int(o[r]), int(o[r + 1])):
                acc = fn(acc, int(v[r]), int(nb[j]), None if x is None else int(x[j]))
            res.append((int(v[r]), acc))
        return res

    def stats(self, op) -> dict:
        s = GsSliceWindowStats()
        call("gs_slice_stats", self.handle, _op(op), ctypes.byref(s))
        return {"n_vertices": int(s.n_vertices), "n_entries": int(s.n_entries), "max_row": int(s.max_row),
                "checksum": int(s.checksum)}

    # ---- every window of a stream ----
    def reduce_windows(self, src, dst, values, window_edges: int, op, out=None):
        """Every window of ``window_edges`` edges (the last may be shorter) in one call with one host
        wait: ``(records, stats)``, records a list of per-window ``(vertices, values)`` and stats one
        (n_vertices, n_entries, max_row, checksum) per window. ``out``: a pair of arrays or device
        tensors for the concatenated records; ``(window_offsets, stats)`` is returned then."""
        w = int(window_edges)
        if w <= 0:
            raise ValueError("window_edges must be positive")
        code = _op(op)
        ps, pd, pv, n, keep = self._edges(src, dst, values)
        nw = (n + w - 1) // w
        offs = np.zeros(nw + 1, dtype=np.uint64)
        stats = np.zeros(nw, dtype=_STATS_DTYPE)
        got = U64()
        if out is not None:
            v, x = out
            self._after_torch(v, x)
            cap = min(len(v), len(x))
        else:
            cap = max(self._entries(n), 1)
            v = np.empty(cap, dtype=self._vdtype())
            x = np.empty(cap, dtype=np.int64)
        call("gs_slice_reduce_windows", self.handle, ps, pd, pv, n, w, code, _out_ptr(v), _out_ptr(x), cap,
             offs.ctypes.data_as(ctypes.c_void_p), stats.ctypes.data_as(ctypes.c_void_p), nw, ctypes.byref(got))
        del keep
        self._n = n - (nw - 1) * w if nw else 0
        self._has_values = values is not None
        nw = int(got.value)
        if out is not None:
            return offs[:nw + 1], stats[:nw]
        o = offs.astype(np.int64)
        return [(v[o[k]:o[k + 1]], x[o[k]:o[k + 1]]) for k in range(nw)], stats[:nw]


def slice_stream(stream, window_edges: Optional[int] = None, direction: str = "out", time_millis: int = 0,
                 vertex_capacity: Optional[int] = None, id_bits: int = 64, device: int = 0):
    """SimpleEdgeStream.slice: one ``SnapshotStream`` view per window, in window order. The views
    share one handle: a view is valid until the next one is taken."""
    if len(stream) == 0:
        return
    cap = int(vertex_capacity) if vertex_capacity else int(max(stream.src.max(), stream.dst.max())) + 1
    vals = getattr(stream, "values", None)
    with SnapshotStream(cap, direction, id_bits, device) as ss:
        for w in stream.windows(time_millis, window_edges):
            yield ss.window(stream.src[w], stream.dst[w], None if vals is None else vals[w])
