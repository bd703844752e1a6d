"""Streaming vertex degrees and the degree distribution on the device (include/gsgpu.h gs_deg_*):
Python mirror of the reference's ``SimpleEdgeStream.getDegrees / getInDegrees / getOutDegrees``
(SimpleEdgeStream.java:413-478) and ``example/DegreeDistribution.java`` (:70-132), the reference's
consumer of ``EventType``: edge additions AND deletions.

``DegreeSummary`` holds ``degree[v]`` of every vertex with degree > 0 and ``count[d]``, the number
of vertices of degree ``d``. An event ``(src, dst, add)`` is two vertex events in stream order, each
of them ``x -> max(x + change, 0)`` on its vertex's degree. The library works in count windows; after
a window the summary equals the reference's maps after the same prefix of the stream. The
per-window emissions are deltas: the keys whose value after the window differs from before it, with
the new value — the reference's last record of that key within the window; its records for keys
that end the window where they began are not reproduced (with one-event windows: count[1] when one
vertex leaves degree 1 and another enters it).
"""
from __future__ import annotations

import ctypes
from typing import Iterator, List, Optional, Tuple

import numpy as np

from . import _abi
from ._abi import GsDegWindowStats, call
from .summary import _as_torch_stream, _buf, _current_raw_stream, _first_cuda_tensor, _is_torch, _stream_ptr

U64 = ctypes.c_uint64
_PATHS = {None: 0, "sort": _abi.GS_DEG_SORT_ALL, "count": _abi.GS_DEG_COUNT}
_DIRS = {"all": 0, "out": _abi.GS_DEG_OUT, "in": _abi.GS_DEG_IN}
_STATS_DTYPE = np.dtype([("n_vertices", np.uint64), ("n_degrees", np.uint64), ("max_degree", np.uint64),
                         ("checksum", np.uint64)])


def _events(add, n: int):
    """(pointer, keepalive) of a nullable event array: 1 = addition, 0 = deletion."""
    if add is None:
        return None, None
    if _is_torch(add):
        import torch
        if add.dtype not in (torch.uint8, torch.bool) or not add.is_contiguous():
            raise TypeError("events: a contiguous uint8 / bool tensor is expected")
        if add.numel() != n:
            raise ValueError("events: %d entries for %d edges" % (add.numel(), n))
        return ctypes.c_void_p(add.data_ptr()), add
    a = np.ascontiguousarray(np.asarray(add).astype(bool).astype(np.uint8))
    if a.size != n:
        raise ValueError("events: %d entries for %d edges" % (a.size, n))
    return a.ctypes.data_as(ctypes.c_void_p), a


class DegreeSummary:
    """Degrees and their distribution; dense ids in [0, vertex_capacity), capacity <= 2^32 - 1.

    ``direction``: "all" (both ends of an edge), "out" (sources) or "in" (targets).
    ``path``: "sort" sends every vertex event through the exact (sort and compose) path, "count"
    counts per vertex and sorts only the events of vertices a window could clamp; None: the
    library's default (the one measured faster: "sort"). The results are the same.
    ``dense_degrees``: ``count[d]`` is a dense array below it (0: the library's default)."""

    def __init__(self, vertex_capacity: int, id_bits: int = 64, device: int = 0, stream=None,
                 direction: str = "all", path: Optional[str] = None, dense_degrees: int = 0):
        if direction not in _DIRS:
            raise ValueError("direction must be 'all', 'in' or 'out'")
        if path not in _PATHS:
            raise ValueError("path must be None, 'sort' or 'count'")
        self.capacity = int(vertex_capacity)
        self.id_bits = int(id_bits)
        self.direction = direction
        self.path = path
        self._h = None
        h = ctypes.c_void_p()
        call("gs_deg_create", ctypes.byref(h), self.capacity, self.id_bits, int(device),
             _DIRS[direction] | _PATHS[path], int(dense_degrees))
        self._h = h
        self._hs: Optional[int] = None
        if stream is not None:
            self.set_stream(stream)

    @property
    def handle(self) -> ctypes.c_void_p:
        if self._h is None:
            raise RuntimeError("DegreeSummary is closed")
        return self._h

    def close(self) -> None:
        if getattr(self, "_h", None) is not None:
            _abi.lib().gs_deg_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - GC timing
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self) -> "DegreeSummary":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def set_stream(self, stream) -> None:
        call("gs_deg_set_stream", self.handle, _stream_ptr(stream))
        self._hs = None

    def _stream(self) -> int:
        if self._hs is None:
            s = ctypes.c_void_p()
            call("gs_deg_get_stream", self.handle, ctypes.byref(s))
            self._hs = int(s.value or 0)
        return self._hs

    def _after_torch(self, *objs) -> None:
        """Device tensors a call reads were produced in torch's stream order: the handle's stream
        waits for torch's current stream first (an event, no host wait), as TriangleCounter does.
        Every fold here ends with a host wait on the handle's stream, so nothing is owed back."""
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
        call("gs_deg_sync", self.handle)

    def reset(self) -> None:
        call("gs_deg_reset", self.handle)

    def _edges(self, src, dst, add):
        ps, ks, n = _buf(src, self.id_bits, "src")
        pd, kd, m = _buf(dst, self.id_bits, "dst")
        if n != m:
            raise ValueError("src and dst lengths differ (%d, %d)" % (n, m))
        pa, ka = _events(add, n)
        self._after_torch(ks, kd, ka)
        return ps, pd, pa, n, (ks, kd, ka)

    # ---- folding ----
    def fold_window(self, src, dst, add=None) -> None:
        """One window: fold its events and close it."""
        ps, pd, pa, n, keep = self._edges(src, dst, add)
        call("gs_deg_fold_window", self.handle, ps, pd, pa, n)
        del keep

    def fold_windows(self, src, dst, window_edges: int, add=None) -> np.ndarray:
        """Every window of ``window_edges`` events (the last may be shorter) in one call; returns one
        (n_vertices, n_degrees, max_degree, checksum) record per window."""
        w = int(window_edges)
        if w <= 0:
            raise ValueError("window_edges must be positive")
        ps, pd, pa, n, keep = self._edges(src, dst, add)
        nw = (n + w - 1) // w
        stats = np.zeros(nw, dtype=_STATS_DTYPE)
        got = U64()
        call("gs_deg_fold_windows", self.handle, ps, pd, pa, n, w, stats.ctypes.data_as(ctypes.c_void_p), nw,
             ctypes.byref(got))
        del keep
        return stats[:int(got.value)]

    # ---- the summary ----
    def stats(self) -> dict:
        s = GsDegWindowStats()
        call("gs_deg_stats", self.handle, ctypes.byref(s))
        return {"n_vertices": int(s.n_vertices), "n_degrees": int(s.n_degrees), "max_degree": int(s.max_degree),
                "checksum": int(s.checksum)}

    def path_counts(self) -> dict:
        """Since the handle was made: windows folded, windows that took the exact path, vertex
        events, and vertex events that were sorted."""
        w, ew, e, ee = U64(), U64(), U64(), U64()
        call("gs_deg_path_counts", self.handle, ctypes.byref(w), ctypes.byref(ew), ctypes.byref(e), ctypes.byref(ee))
        return {"windows": int(w.value), "exact_windows": int(ew.value), "vertex_events": int(e.value),
                "exact_events": int(ee.value)}

    def _pairs(self, fn: str, kdtype, vdtype, guess: int):
        cap = max(int(guess), 16)
        while True:
            k = np.empty(cap, dtype=kdtype)
            v = np.empty(cap, dtype=vdtype)
            n = U64()
            rc = getattr(_abi.lib(), fn)(self.handle, k.ctypes.data_as(ctypes.c_void_p), v.ctypes.data_as(ctypes.c_void_p),
                                         cap, ctypes.byref(n))
            if rc == _abi.GS_ERR_CAPACITY and int(n.value) > cap:
                cap = int(n.value)
                continue
            if rc != _abi.GS_OK:
                msg = _abi.lib().gs_last_error()
                raise _abi.GsError(rc, fn, msg.decode() if msg else "")
            return k[:int(n.value)], v[:int(n.value)]

    def _vdtype(self):
        return np.uint32 if self.id_bits == 32 else np.int64

    def degrees(self) -> Tuple[np.ndarray, np.ndarray]:
        """(vertices, degrees) of every vertex with degree > 0, ordered by vertex."""
        return self._pairs("gs_deg_emit_degrees", self._vdtype(), np.uint32, 1024)

    def degrees_delta(self) -> Tuple[np.ndarray, np.ndarray]:
        """The last window's degree delta: (vertices, new degrees; 0 = removed), ordered by vertex."""
        return self._pairs("gs_deg_emit_degrees_delta", self._vdtype(), np.uint32, 1024)

    def distribution(self) -> Tuple[np.ndarray, np.ndarray]:
        """(degrees, counts) of every degree with count > 0, ordered by degree."""
        return self._pairs("gs_deg_emit_distribution", np.uint32, np.uint64, 256)

    def distribution_delta(self) -> Tuple[np.ndarray, np.ndarray]:
        """The last window's distribution delta: (degrees, new counts; may be 0), ordered by degree."""
        return self._pairs("gs_deg_emit_distribution_delta", np.uint32, np.uint64, 256)

    def find(self, ids) -> np.ndarray:
        """Degrees of ``ids``; 0 for an absent vertex."""
        p, keep, n = _buf(ids, self.id_bits, "ids")
        self._after_torch(keep)
        out = np.zeros(n, dtype=np.uint32)
        call("gs_deg_find", self.handle, p, out.ctypes.data_as(ctypes.c_void_p), n)
        del keep
        return out

    # ---- the Merger's checkpoint ----
    def snapshot(self) -> Tuple[np.ndarray, np.ndarray]:
        v, d = self.degrees()
        return v.copy(), d.copy()

    def restore(self, vertices, degrees) -> None:
        """The summary becomes the snapshot's (pairs in any order); distribution, statistics and
        checksum are rebuilt on the device."""
        pv, kv, n = _buf(vertices, self.id_bits, "vertices")
        d = np.ascontiguousarray(np.asarray(degrees, dtype=np.uint32))
        if d.size != n:
            raise ValueError("vertices and degrees lengths differ (%d, %d)" % (n, d.size))
        call("gs_deg_restore", self.handle, pv, d.ctypes.data_as(ctypes.c_void_p), n)
        del kv


class DegreeDistribution:
    """DegreeDistribution (example/DegreeDistribution.java:52-59) over a ``SimpleEdgeStream`` with
    ``events``: per count window, the distribution delta as a list of ``(degree, count)``."""

    def __init__(self, window_edges: int = 1, vertex_capacity: Optional[int] = None, id_bits: int = 64,
                 device: int = 0, path: Optional[str] = None, dense_degrees: int = 0):
        if int(window_edges) <= 0:
            raise ValueError("window_edges must be positive")
        self.window_edges = int(window_edges)
        self.vertex_capacity = vertex_capacity
        self.id_bits = int(id_bits)
        self.device = int(device)
        self.path = path
        self.dense_degrees = int(dense_degrees)
        self._summary: Optional[DegreeSummary] = None
        self._restored = None

    def snapshotState(self, checkpointId: int = 0, timestamp: int = 0) -> list:
        """The vertex -> degree map as (vertices, degrees); an empty list outside a run."""
        if self._summary is None:
            return []
        return [self._summary.snapshot()]

    def restoreState(self, state: list) -> None:
        """The next run() starts from this snapshot."""
        self._restored = state[0] if state else None

    def _capacity(self, stream) -> int:
        if self.vertex_capacity:
            return int(self.vertex_capacity)
        cap = int(max(stream.src.max(), stream.dst.max())) + 1 if len(stream) else 1
        if self._restored is not None and len(self._restored[0]):
            cap = max(cap, int(np.asarray(self._restored[0]).max()) + 1)
        return cap

    def run(self, stream) -> Iterator[List[Tuple[int, int]]]:
        ds = DegreeSummary(self._capacity(stream), self.id_bits, self.device, path=self.path,
                           dense_degrees=self.dense_degrees)
        self._summary = ds
        try:
            if self._restored is not None:
                ds.restore(*self._restored)
            ev = getattr(stream, "events", None)
            for w in stream.windows(0, self.window_edges):
                ds.fold_window(stream.src[w], stream.dst[w], None if ev is None else ev[w])
                d, c = ds.distribution_delta()
                yield list(zip(d.tolist(), c.tolist()))
        finally:
            self._summary = None
            ds.close()


def degree_stream(stream, direction: str, window_edges: int = 1, vertex_capacity: Optional[int] = None,
                  id_bits: int = 64, device: int = 0, path: Optional[str] = None) -> Iterator[List[Tuple[int, int]]]:
    """getDegrees / getInDegrees / getOutDegrees: per count window, the degree delta as
    ``(vertex, degree)`` pairs ordered by vertex (additions only, as the reference's operators)."""
    if int(window_edges) <= 0:
        raise ValueError("window_edges must be positive")
    cap = int(vertex_capacity) if vertex_capacity else (int(max(stream.src.max(), stream.dst.max())) + 1 if len(stream) else 1)
    with DegreeSummary(cap, id_bits, device, direction=direction, path=path) as ds:
        for w in stream.windows(0, int(window_edges)):
            ds.fold_window(stream.src[w], stream.dst[w])
            v, d = ds.degrees_delta()
            yield list(zip(v.tolist(), d.tolist()))
