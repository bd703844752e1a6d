"""CPU: the triangle oracles agree with the reference's known answer and with each other, and the
gs_tri_* calls that need no device validate their arguments."""
import ctypes
import json
import os

import numpy as np
import pytest

import gsgpu
from gsgpu import _abi
from triangles_oracle import (dense_count, drop_self_loops, literal_window_count, random_multigraph,
                              sorted_adjacency_count)

KAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "window_triangles_kat.json")


def kat():
    with open(KAT) as f:
        return json.load(f)


def test_literal_count_gives_the_reference_known_answer():
    k = kat()
    e = np.asarray(k["edges"], dtype=np.int64)
    assert e.shape == (19, 3)
    wid = e[:, 2] // k["window_ms"]
    got = []
    for w in np.unique(wid):
        sel = wid == w
        got.append([literal_window_count(e[sel, 0], e[sel, 1]), int((w + 1) * k["window_ms"] - 1)])
    assert [int(sel.sum()) for sel in (wid == 0, wid == 1, wid == 2)] == [6, 8, 5]
    assert got == k["expected"] == [[2, 399], [3, 799], [2, 1199]]


@pytest.mark.parametrize("nv,n", [(8, 40), (64, 600), (300, 6000)])
def test_literal_equals_dense_on_random_multigraphs(nv, n):
    src, dst = random_multigraph(nv, n, seed=nv + n)
    assert np.any(src == dst), "the stream is meant to hold self-loops"
    s, d = drop_self_loops(src, dst)                      # removed before the literal function runs
    assert not np.any(s == d)
    total, local = dense_count(src, dst, nv)
    assert literal_window_count(s, d) == total
    assert total > 0
    assert int(local.sum()) == 3 * total
    t2, l2 = sorted_adjacency_count(src, dst, nv)
    assert t2 == total
    np.testing.assert_array_equal(l2, local)


def test_dense_count_of_a_clique_and_a_path():
    n = 12
    i, j = np.triu_indices(n, 1)
    total, local = dense_count(i, j, n)
    assert total == n * (n - 1) * (n - 2) // 6
    assert local.tolist() == [(n - 1) * (n - 2) // 2] * n
    assert dense_count(np.arange(9), np.arange(1, 10), 10)[0] == 0
    assert literal_window_count(np.arange(9), np.arange(1, 10)) == 0


def test_tri_argument_validation_without_device():
    L = gsgpu.lib()
    h = ctypes.c_void_p()
    bad = _abi.GS_ERR_INVALID
    assert L.gs_tri_create(None, 100, 32, 0, 0) == bad
    assert L.gs_tri_create(ctypes.byref(h), 100, 16, 0, 0) == bad
    assert b"id_bits" in L.gs_last_error()
    assert L.gs_tri_create(ctypes.byref(h), 0, 32, 0, 0) == bad
    assert L.gs_tri_create(ctypes.byref(h), (1 << 32) + 1, 64, 0, 0) == bad
    assert L.gs_tri_create(ctypes.byref(h), 100, 32, 0, 2) == bad
    assert b"flags" in L.gs_last_error()
    assert h.value is None
    nw, tot = ctypes.c_uint64(), ctypes.c_uint64()
    assert L.gs_tri_count_windows(None, None, None, 0, 1, None, 0, ctypes.byref(nw)) == bad
    assert L.gs_tri_count_local(None, None, None, 0, None, ctypes.byref(tot), None) == bad
    assert L.gs_tri_set_stream(None, None) == bad
    assert L.gs_tri_get_stream(None, None) == bad
    assert L.gs_tri_sync(None) == bad


def test_tri_destroy_null_is_ok():
    assert gsgpu.lib().gs_tri_destroy(None) == _abi.GS_OK


def test_python_surface_is_exported():
    assert gsgpu.TriangleCounter is not None and gsgpu.WindowTriangles is not None
    with pytest.raises(ValueError):
        gsgpu.TriangleCounter(10, orient="rank")
