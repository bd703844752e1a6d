"""Exact triangle counts of edge windows on the device (include/gsgpu.h gs_tri_*): Python mirror of
the reference's ``example/WindowTriangles.java`` (:60-65: ``slice(window, ALL)`` ->
``GenerateCandidateEdges`` -> ``CountTriangles`` -> ``timeWindowAll.sum``).

``TriangleCounter`` counts the triangles of the simple undirected graph of a batch of edges
(repeated edges and both directions count once, self-loops are ignored), of every window of a
stream in one call, or per vertex (the final counters of ``example/ExactTriangleCount.java`` for a
stream without repeated edges). ``WindowTriangles(windowTime)`` runs over a ``SimpleEdgeStream``
and yields the reference's emission ``(count, window.maxTimestamp())`` per non-empty window.
"""
from __future__ import annotations

import ctypes
from typing import Iterator, Optional, Tuple

import numpy as np

from . import _abi
from ._abi import call
from .summary import _as_torch_stream, _buf, _current_raw_stream, _first_cuda_tensor, _stream_ptr

U64 = ctypes.c_uint64


class TriangleCounter:
    """Triangle counts of edge batches; dense ids in [0, vertex_capacity), capacity <= 2^32.

    ``orient="degree"`` (default) directs every edge from its low (degree, id) end to its high
    one, ``orient="id"`` from low id to high id as the reference does; the counts are the same."""

    def __init__(self, vertex_capacity: int, id_bits: int = 64, device: int = 0, stream=None,
                 orient: str = "degree"):
        if orient not in ("degree", "id"):
            raise ValueError("orient must be 'degree' or 'id'")
        self.capacity = int(vertex_capacity)
        self.id_bits = int(id_bits)
        self.orient = orient
        self._h = None
        h = ctypes.c_void_p()
        call("gs_tri_create", ctypes.byref(h), self.capacity, self.id_bits, int(device),
             _abi.GS_TRI_ORIENT_BY_ID if orient == "id" else 0)
        self._h = h
        self._hs: Optional[int] = None
        if stream is not None:
            self.set_stream(stream)

    @property
    def handle(self) -> ctypes.c_void_p:
        if self._h is None:
            raise RuntimeError("TriangleCounter is closed")
        return self._h

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            _abi.lib().gs_tri_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - GC timing
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self) -> "TriangleCounter":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def set_stream(self, stream) -> None:
        call("gs_tri_set_stream", self.handle, _stream_ptr(stream))
        self._hs = None

    def _stream(self) -> int:
        if self._hs is None:
            s = ctypes.c_void_p()
            call("gs_tri_get_stream", self.handle, ctypes.byref(s))
            self._hs = int(s.value or 0)
        return self._hs

    def _after_torch(self, *objs) -> None:
        """Device tensors a call reads were produced in torch's stream order: the handle's stream
        waits for torch's current stream first (an event, no host wait), as DisjointSet does.
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
        call("gs_tri_sync", self.handle)

    def _edges(self, src, dst):
        ps, ks, n = _buf(src, self.id_bits, "src")
        pd, kd, m = _buf(dst, self.id_bits, "dst")
        if n != m:
            raise ValueError("src and dst lengths differ (%d, %d)" % (n, m))
        self._after_torch(ks, kd)
        return ps, pd, n, (ks, kd)

    def count_windows(self, src, dst, window_edges: int) -> np.ndarray:
        """Triangles of every window of ``window_edges`` edges (the last may be shorter), counted
        in one call with one host wait at its end."""
        w = int(window_edges)
        if w <= 0:
            raise ValueError("window_edges must be positive")
        ps, pd, n, keep = self._edges(src, dst)
        nw = (n + w - 1) // w
        counts = np.zeros(nw, dtype=np.uint64)
        got = U64()
        call("gs_tri_count_windows", self.handle, ps, pd, n, w, counts.ctypes.data_as(ctypes.c_void_p), nw,
             ctypes.byref(got))
        del keep
        return counts[:int(got.value)]

    def count(self, src, dst) -> int:
        """Triangles of the simple undirected graph of these edges."""
        return self._local(src, dst, False)[0]

    def local(self, src, dst) -> Tuple[int, np.ndarray]:
        """(total, per-vertex counts): a vertex's count is the number of triangles it is in, so
        the counts sum to 3 x total."""
        total, loc, _ = self._local(src, dst, True)
        return total, loc

    def simple_edges(self, src, dst) -> int:
        """Distinct undirected edges without self-loops among these edges."""
        return self._local(src, dst, False)[2]

    def _local(self, src, dst, want_local: bool):
        ps, pd, n, keep = self._edges(src, dst)
        loc = np.zeros(self.capacity, dtype=np.uint64) if want_local else None
        total, simple = U64(), U64()
        call("gs_tri_count_local", self.handle, ps, pd, n,
             loc.ctypes.data_as(ctypes.c_void_p) if want_local else None, ctypes.byref(total), ctypes.byref(simple))
        del keep
        return int(total.value), loc, int(simple.value)


class WindowTriangles:
    """WindowTriangles (example/WindowTriangles.java:60-65) over a ``SimpleEdgeStream``: one
    ``(count, maxTimestamp)`` per non-empty window, in window order.

    Windows come from ``SimpleEdgeStream.windows``. With timestamps a window's maxTimestamp is
    ``(t // windowTime + 1) * windowTime - 1`` (TimeWindow.maxTimestamp of Flink's tumbling
    window); with ``window_edges`` the edge index is the timestamp: window k ends at
    ``(k + 1) * window_edges - 1``."""

    def __init__(self, windowTime: int, *, window_edges: Optional[int] = None, vertex_capacity: Optional[int] = None,
                 id_bits: int = 64, device: int = 0, orient: str = "degree"):
        self.time_millis = int(windowTime)
        self.window_edges = window_edges
        self.vertex_capacity = vertex_capacity
        self.id_bits = int(id_bits)
        self.device = int(device)
        self.orient = orient

    def _capacity(self, stream) -> int:
        if self.vertex_capacity:
            return int(self.vertex_capacity)
        return int(max(stream.src.max(), stream.dst.max())) + 1

    def run(self, stream) -> Iterator[Tuple[int, int]]:
        if len(stream) == 0:
            return
        timed = stream.timestamps is not None and not self.window_edges
        wins = stream.windows(self.time_millis, self.window_edges)
        with TriangleCounter(self._capacity(stream), self.id_bits, self.device, orient=self.orient) as tc:
            if timed:                                   # windows of any length: one call each
                for w in wins:
                    t = int(stream.timestamps[w.start])
                    yield tc.count(stream.src[w], stream.dst[w]), (t // self.time_millis + 1) * self.time_millis - 1
                return
            we = int(self.window_edges) if self.window_edges else len(stream)
            counts = tc.count_windows(stream.src, stream.dst, we)
        for k, c in enumerate(counts.tolist()):
            yield int(c), (k + 1) * we - 1
