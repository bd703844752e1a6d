"""GPU parity of the per-window triangle counts (gs_tri_*): the reference's known answer
(WindowTrianglesITCase) exactly, random multigraph streams equal to the CPU oracles in every
window, per-vertex counts, rows longer than one LDS tile, the bin boundaries and the edge cases.
Integer path: every comparison is exact."""
import ctypes
import functools
import json
import os
import threading

import numpy as np
import pytest

from gsgpu import GsError, SimpleEdgeStream, TriangleCounter, WindowTriangles
from gsgpu import _abi
from triangles_oracle import (dense_count, drop_self_loops, literal_window_count, random_multigraph,
                              sorted_adjacency_count)

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ORIENTS = ["degree", "id"]


def test_reference_known_answer():
    k = json.load(open(os.path.join(GOLD, "window_triangles_kat.json")))
    e = np.asarray(k["edges"], dtype=np.int64)
    stream = SimpleEdgeStream(e[:, 0], e[:, 1], e[:, 2])
    got = [[c, t] for c, t in stream.aggregate(WindowTriangles(k["window_ms"]))]
    assert got == [[2, 399], [3, 799], [2, 1199]] == k["expected"]
    assert [[c, t] for c, t in WindowTriangles(k["window_ms"], orient="id", id_bits=32).run(stream)] == k["expected"]


STREAMS = [(8, 40, 40), (64, 610, 150), (300, 6000, 1000), (1000, 20000, 20000),
           (1 << 14, 1 << 18, 1 << 16)]               # (nv, n, W); n = 610: the last window is short


@functools.lru_cache(maxsize=None)
def _stream_and_oracle(nv, n, W):
    """The stream (self-loops and repeated edges kept) and every window's oracle count."""
    src, dst = random_multigraph(nv, n, seed=7 * nv + n)
    want = []
    for lo in range(0, n, W):
        s, d = src[lo:lo + W], dst[lo:lo + W]
        if nv <= 1000:
            total = dense_count(s, d, nv)[0]
            assert literal_window_count(*drop_self_loops(s, d)) == total
        else:
            total = sorted_adjacency_count(s, d, nv)[0]
        want.append(total)
    src.setflags(write=False)
    dst.setflags(write=False)
    return src, dst, tuple(want)


@pytest.mark.parametrize("orient", ORIENTS)
@pytest.mark.parametrize("id_bits", [32, 64])
@pytest.mark.parametrize("nv,n,W", STREAMS)
def test_random_streams_equal_the_oracle(nv, n, W, id_bits, orient):
    src, dst, want = _stream_and_oracle(nv, n, W)
    assert np.any(src == dst) and len(want) == -(-n // W)
    assert sum(want) > 0
    with TriangleCounter(nv, id_bits=id_bits, orient=orient) as tc:
        got = tc.count_windows(src, dst, W)
        assert got.dtype == np.uint64
        assert got.tolist() == list(want)
        each = [tc.count(src[lo:lo + W], dst[lo:lo + W]) for lo in range(0, n, W)]
        assert each == list(want)
    if n % W:
        assert n - (len(want) - 1) * W < W                  # the last window is short


@pytest.mark.parametrize("orient", ORIENTS)
def test_window_triangles_with_edge_count_windows(orient):
    nv, n, W = 64, 610, 150
    src, dst, want = _stream_and_oracle(nv, n, W)
    out = list(SimpleEdgeStream(src, dst).aggregate(WindowTriangles(0, window_edges=W, vertex_capacity=nv, orient=orient)))
    assert out == [(c, (k + 1) * W - 1) for k, c in enumerate(want)]


@pytest.mark.parametrize("orient", ORIENTS)
@pytest.mark.parametrize("id_bits", [32, 64])
def test_local_counts_random(id_bits, orient):
    nv, n = 300, 6000
    src, dst = random_multigraph(nv, n, seed=11)
    total, local = dense_count(src, dst, nv)
    with TriangleCounter(nv, id_bits=id_bits, orient=orient) as tc:
        got_total, got_local = tc.local(src, dst)
        assert tc.simple_edges(src, dst) == len(set(zip(np.minimum(src, dst).tolist(), np.maximum(src, dst).tolist()))
                                                - {(v, v) for v in range(nv)})
    assert got_total == total
    np.testing.assert_array_equal(got_local, local)
    assert int(got_local.sum()) == 3 * total


@pytest.mark.parametrize("orient", ORIENTS)
def test_local_counts_clique(orient):
    n = 200
    i, j = np.triu_indices(n, 1)
    with TriangleCounter(n, orient=orient) as tc:
        total, local = tc.local(j, i)                       # (given high -> low: the direction is ignored)
        assert tc.count(i, j) == 1313400
    assert total == 1313400 == n * (n - 1) * (n - 2) // 6
    assert local.tolist() == [19701] * n
    assert int(local.sum()) == 3 * total


@pytest.mark.parametrize("orient", ORIENTS)
def test_rows_longer_than_one_lds_tile(orient):
    """Hub 0 joined to 1..44,999 plus the path 1-2-...-44,999: one triangle (0, i, i + 1) per path
    edge = 44,998. Under orient="id" the hub's out-row holds 44,999 ids, more than the 40,960
    words 160 KiB of LDS can hold, so whatever the tile size the tile loop wraps."""
    L = 44999
    leaves = np.arange(1, L + 1, dtype=np.int64)
    src = np.concatenate([np.zeros(L, dtype=np.int64), leaves[:-1]])
    dst = np.concatenate([leaves, leaves[1:]])
    with TriangleCounter(L + 1, orient=orient) as tc:
        assert tc.count(src, dst) == 44998
        total, local = tc.local(src, dst)
    assert total == 44998
    assert local[0] == 44998 and local[1] == 1 and local[L] == 1
    assert np.all(local[2:L] == 2)


@pytest.mark.parametrize("orient", ORIENTS)
def test_bin_boundaries(orient):
    """Fans (a hub, its leaves, the path through the leaves: leaves - 1 triangles) whose hub rows
    have 63, 64, 65, 255, 256 and 257 entries under orient="id", all in one window."""
    sizes = [63, 64, 65, 255, 256, 257]
    src, dst, hubs, base = [], [], [], 0
    for L in sizes:
        leaves = np.arange(base + 1, base + L + 1, dtype=np.int64)
        src += [np.full(L, base, dtype=np.int64), leaves[:-1]]
        dst += [leaves, leaves[1:]]
        hubs.append(base)
        base += L + 1
    src, dst = np.concatenate(src), np.concatenate(dst)
    with TriangleCounter(base, orient=orient) as tc:
        assert tc.count(src, dst) == sum(L - 1 for L in sizes)
        total, local = tc.local(src, dst)
        assert tc.count_windows(src, dst, src.size).tolist() == [total]
    assert total == sum(L - 1 for L in sizes)
    assert local[hubs].tolist() == [L - 1 for L in sizes]
    assert int(local.sum()) == 3 * total


@pytest.mark.parametrize("orient", ORIENTS)
def test_windows_without_triangles_and_empty_input(orient):
    path_s, path_d = np.arange(0, 99), np.arange(1, 100)
    a, b = np.meshgrid(np.arange(0, 30), np.arange(30, 70))   # a complete bipartite block
    with TriangleCounter(100, orient=orient) as tc:
        assert tc.count(path_s, path_d) == 0
        assert tc.count(a.ravel(), b.ravel()) == 0
        assert tc.count_windows(np.concatenate([path_s, a.ravel()]), np.concatenate([path_d, b.ravel()]), 99).tolist() \
            == [0] * -(-(99 + 1200) // 99)
        assert tc.count_windows(np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64), 10).size == 0
        assert tc.count(np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64)) == 0
        assert tc.count(np.array([5, 5]), np.array([5, 5])) == 0   # self-loops only
        with pytest.raises(ValueError):
            tc.count_windows(path_s, path_d, 0)
        nw = ctypes.c_uint64()
        assert _abi.lib().gs_tri_count_windows(tc.handle, None, None, 5, 0, None, 0, ctypes.byref(nw)) == _abi.GS_ERR_INVALID
    assert list(WindowTriangles(100).run(SimpleEdgeStream([], []))) == []
    assert list(WindowTriangles(100).run(SimpleEdgeStream([0, 1, 2], [1, 2, 3], [0, 50, 250]))) == [(0, 99), (0, 299)]


@pytest.mark.parametrize("id_bits", [32, 64])
def test_id_equal_to_capacity_is_a_range_error(id_bits):
    src, dst, want = _stream_and_oracle(64, 610, 150)
    bad_s = src.copy()
    bad_s[200] = 64
    with TriangleCounter(64, id_bits=id_bits) as tc:
        with pytest.raises(GsError) as ei:
            tc.count_windows(bad_s, dst, 150)
        assert ei.value.code == _abi.GS_ERR_RANGE
        with pytest.raises(GsError) as ei:
            tc.count(bad_s, dst)
        assert ei.value.code == _abi.GS_ERR_RANGE
        if id_bits == 64:
            neg = src.copy()
            neg[3] = -1
            with pytest.raises(GsError) as ei:
                tc.count(neg, dst)
            assert ei.value.code == _abi.GS_ERR_RANGE
        assert tc.count_windows(src, dst, 150).tolist() == list(want)   # the handle is as good as new


def test_capacity_one_short_writes_nothing():
    src, dst, want = _stream_and_oracle(64, 610, 150)
    mark = np.uint64(0xDEADBEEF)
    counts = np.full(len(want), mark, dtype=np.uint64)
    nw = ctypes.c_uint64()
    with TriangleCounter(64) as tc:
        rc = _abi.lib().gs_tri_count_windows(tc.handle, src.ctypes.data_as(ctypes.c_void_p), dst.ctypes.data_as(ctypes.c_void_p),
                                             src.size, 150, counts.ctypes.data_as(ctypes.c_void_p), len(want) - 1,
                                             ctypes.byref(nw))
        assert rc == _abi.GS_ERR_CAPACITY
        assert nw.value == len(want)
        assert np.all(counts == mark)
        rc = _abi.lib().gs_tri_count_windows(tc.handle, src.ctypes.data_as(ctypes.c_void_p), dst.ctypes.data_as(ctypes.c_void_p),
                                             src.size, 150, counts.ctypes.data_as(ctypes.c_void_p), len(want),
                                             ctypes.byref(nw))
        assert rc == _abi.GS_OK and counts.tolist() == list(want)


@pytest.mark.parametrize("id_bits", [32, 64])
def test_host_and_device_inputs_agree(id_bits):
    import torch
    nv, n, W = 300, 6000, 1000
    src, dst, want = _stream_and_oracle(nv, n, W)
    dt = torch.int32 if id_bits == 32 else torch.int64
    ds = torch.from_numpy(src.copy()).to("cuda").to(dt)
    dd = torch.from_numpy(dst.copy()).to("cuda").to(dt)
    with TriangleCounter(nv, id_bits=id_bits) as tc:
        host = tc.count_windows(src, dst, W)
        dev = tc.count_windows(ds, dd, W)
        assert host.tolist() == dev.tolist() == list(want)
        th, lh = tc.local(src, dst)
        td, ld = tc.local(ds, dd)
        assert th == td
        np.testing.assert_array_equal(lh, ld)
    with TriangleCounter(nv, id_bits=id_bits, stream=torch.cuda.current_stream()) as tc:
        assert tc.count_windows(ds, dd, W).tolist() == list(want)


def test_two_handles_on_two_streams():
    a = _stream_and_oracle(300, 6000, 1000)
    b = _stream_and_oracle(1000, 20000, 20000)
    out, err = {}, []

    def work(name, nv, data, W, orient):
        try:
            src, dst, _ = data
            with TriangleCounter(nv, orient=orient) as tc:       # its own stream
                out[name] = [tc.count_windows(src, dst, W).tolist() for _ in range(3)]
        except Exception as e:  # pragma: no cover - reported below
            err.append(e)

    ts = [threading.Thread(target=work, args=("a", 300, a, 1000, "degree")),
          threading.Thread(target=work, args=("b", 1000, b, 20000, "id"))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not err, err
    assert out["a"] == [list(a[2])] * 3
    assert out["b"] == [list(b[2])] * 3
