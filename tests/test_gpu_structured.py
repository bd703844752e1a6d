"""GPU parity on structured graphs (tests/structured_streams.py) at the odd capacity 2^20 + 3, with the
library's production defaults, every comparison bit-exact against the C oracle (which
tests/test_structured_oracle.py checks against scipy): per window by checksum(), at the end by
dense() and stats().

What the families reach that random streams do not (csrc/cc_kernels.hpp):
  asc_path, desc_path   a giant that is a path: desc_path re-roots it with every edge (the hooked
                        root is the giant's, the s_ren rename in every close), asc_path hangs one
                        new vertex under it per edge, up to the last id
  shuffled_path,        mature windows with no giant (sample_giant / mode_of_samples below 25 %): a
  bitrev_path           full pass every close, hooked-root marks (hb_in), deep trees under path
                        halving; the giant forms in the last windows
  matching              a young forest of N/2 roots, never a giant, then chained into one path
  star_max_hub          the root renamed by every smaller leaf, all hooks on one parent word
  binary_tree_desc      a tree that grows downwards in ids: the root drops at every level
  comb                  a giant that is a comb (the giant filter, hot and warm admission and claims
                        against a path-shaped giant), outside components that attach late
                        (k_compress's incremental branch, sbits & ~gbits and cbits), 64 root drops
  equal_paths           16 mature windows without a giant, list closes with a growing NGL, then
                        large components joining
All of them: the scalar tail (base + 4 > n) and the last words of gbits / sbits / cbits / dbits.
"""
import numpy as np
import pytest

import structured_streams as ss
from gsgpu import DisjointSet
from pyoracle import EMIT_CHECKSUM, dense_checksum

pytestmark = pytest.mark.gpu

N, W = ss.N, ss.W
BIG_W = 1 << 19


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_DEV = {}


def _device_stream(torch, name):
    """The family as int32 device tensors (made once per module)."""
    if name not in _DEV:
        s, d = ss.stream(name)
        _DEV[name] = (torch.from_numpy(s.astype(np.int32)).cuda(), torch.from_numpy(d.astype(np.int32)).cuda())
    return _DEV[name]


def _sums(want):
    return [int(x) for x in want["checksums"]]


def _check_final(ds, want):
    np.testing.assert_array_equal(ds.dense().astype(np.int64), want["final"])
    assert ds.stats() == (want["final_vertices"], want["final_components"])


def _fold_by_window(ds, s, d, window, want):
    n = len(s)
    for w, lo in enumerate(range(0, n, window)):
        ds.fold(s[lo:lo + window], d[lo:lo + window])
        ds.close_window()
        assert ds.checksum()[0] == int(want["checksums"][w]), "window %d" % w
    _check_final(ds, want)


@pytest.mark.parametrize("window", [W, BIG_W], ids=["w2^16", "w2^19"])
@pytest.mark.parametrize("name", ss.FAMILIES)
def test_fold_and_close_every_window(oracle, torch_cuda, name, window):
    """One fold + close_window per window, int32 device arrays; W = 2^16: the young fold, then
    one-edge-per-thread folds with touch logs and list closes; W = 2^19: the four-edges-per-thread
    k_fold with bitmap and full closes and hooked-root marks. Twice on one handle, reset between."""
    want = ss.oracle_windows(oracle, name, window)
    ts, td = _device_stream(torch_cuda, name)
    ds = DisjointSet(N, id_bits=32, stream=torch_cuda.cuda.current_stream())
    _fold_by_window(ds, ts, td, window, want)
    ds.reset()
    assert ds.stats() == (0, 0)
    _fold_by_window(ds, ts, td, window, want)
    ds.close()


@pytest.mark.parametrize("name", ss.FAMILIES)
def test_fold_windows_calls(oracle, torch_cuda, name):
    """gs_cc_fold_windows: the whole stream in one call, then in calls of 3 windows."""
    want = ss.oracle_windows(oracle, name)
    sums = _sums(want)
    ts, td = _device_stream(torch_cuda, name)
    ds = DisjointSet(N, id_bits=32, stream=torch_cuda.cuda.current_stream())
    assert ds.fold_windows(ts, td, W) == len(sums)
    assert ds.checksum()[0] == sums[-1]
    _check_final(ds, want)
    ds.reset()
    for w0 in range(0, len(sums), 3):
        k = min(3, len(sums) - w0)
        assert ds.fold_windows(ts[w0 * W:(w0 + k) * W], td[w0 * W:(w0 + k) * W], W) == k
        assert ds.checksum()[0] == sums[w0 + k - 1], "windows %d-%d" % (w0, w0 + k - 1)
    _check_final(ds, want)
    ds.close()


@pytest.mark.parametrize("name", ss.FAMILIES)
def test_host_int64_arrays(oracle, name):
    """int64 host arrays staged in small chunks (id_bits=64, staging_edges well below a window)."""
    want = ss.oracle_windows(oracle, name)
    s, d = ss.stream(name)
    ds = DisjointSet(N, id_bits=64, staging_edges=10000)
    _fold_by_window(ds, s, d, W, want)
    ds.close()


@pytest.mark.parametrize("name", ss.FAMILIES)
def test_host_int64_pairs(oracle, name):
    """Every window as interleaved int64 host pairs through fold_pairs (the AOS pair fold with
    combine_hooks)."""
    want = ss.oracle_windows(oracle, name)
    s, d = ss.stream(name)
    inter = np.empty(2 * s.size, dtype=np.int64)
    inter[0::2] = s
    inter[1::2] = d
    ds = DisjointSet(N, id_bits=64, staging_edges=10000)
    for w, lo in enumerate(range(0, s.size, W)):
        ds.fold_pairs(inter[2 * lo:2 * (lo + W)], W)
        ds.close_window()
        assert ds.checksum()[0] == int(want["checksums"][w]), "window %d" % w
    _check_final(ds, want)
    ds.close()


@pytest.mark.parametrize("name", ["comb", "equal_paths"])
def test_delta_emission_rebuilds_every_window(oracle, torch_cuda, name):
    """A dense mirror rebuilt from delta() after every window has the oracle's checksum (dbits at an
    odd capacity, through incremental, list and full closes); pairs() after the last window is
    sorted and equal to the final labels (tile count, scan and scatter at an odd capacity)."""
    want = ss.oracle_windows(oracle, name)
    ts, td = _device_stream(torch_cuda, name)
    ds = DisjointSet(N, id_bits=32, stream=torch_cuda.cuda.current_stream())
    mirror = np.full(N, -1, dtype=np.int64)
    for w, lo in enumerate(range(0, ts.numel(), W)):
        ds.fold(ts[lo:lo + W], td[lo:lo + W])
        v, l = ds.delta()
        assert (np.diff(v) > 0).all()
        mirror[v.astype(np.int64)] = l
        assert dense_checksum(mirror)[0] == int(want["checksums"][w]), "window %d" % w
    np.testing.assert_array_equal(mirror, want["final"])
    pv, pl = ds.pairs()
    assert (np.diff(pv) > 0).all()
    np.testing.assert_array_equal(pv, np.nonzero(want["final"] >= 0)[0])
    np.testing.assert_array_equal(pl, want["final"][pv])
    ds.close()


def _strided(v):
    """A monotone map of the ids onto negative ids and ids >= 2^32."""
    return (np.asarray(v, dtype=np.int64) - N // 2) * (1 << 33)


@pytest.mark.parametrize("name", ["comb", "equal_paths", "desc_path"])
def test_sparse_ids(oracle, name):
    """The stream under a monotone strided id map on a sparse=True int64 handle: every window's
    checksum (the oracle's hash-map summary over the mapped ids) and the final pairs, which are the
    mapped labels (a monotone map keeps every component's minimum)."""
    s, d = ss.stream(name)
    ms, md = _strided(s), _strided(d)
    assert ms.min() < 0 and ms.max() >= 1 << 32
    want = oracle.run(ms, md, W, partitions=1, threads=1, emit=EMIT_CHECKSUM)
    final = ss.oracle_windows(oracle, name)["final"]
    ds = DisjointSet(N, id_bits=64, sparse=True)
    for w, lo in enumerate(range(0, s.size, W)):
        ds.fold(ms[lo:lo + W], md[lo:lo + W])
        ds.close_window()
        assert ds.checksum()[0] == int(want["checksums"][w]), "window %d" % w
    pv, pl = ds.pairs()
    seen = np.nonzero(final >= 0)[0]
    np.testing.assert_array_equal(pv, _strided(seen))
    np.testing.assert_array_equal(pl, _strided(final[seen]))
    ds.close()


@pytest.mark.parametrize("name", ["comb", "equal_paths"])
def test_prefilter_three_ranks(oracle, torch_cuda, name):
    """The Merger-rank layout, 3 in-process ranks: k_filter_out against a structured giant."""
    from variant_check import run_prefilter
    s, d = ss.stream(name)
    r = run_prefilter(torch_cuda, oracle, name, s, d, W, N, world=3, want=ss.oracle_windows(oracle, name))
    assert r["ok"], r
    assert r["windows"] == s.size // W


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("cap", ss.ODD_CAPS)
def test_odd_capacities(cap, bits):
    """Capacities with a partial last quad, bitmap word and 1024-id block (2^21 + 1027: a wrapped
    close loop too): dense() against the numpy expectation, find_batch at the edges, twice."""
    s, d, want, windows = ss.odd_capacity_stream(cap)
    ds = DisjointSet(cap, id_bits=bits)
    for _ in range(2):
        for lo, hi in windows:
            ds.fold(s[lo:hi], d[lo:hi])
            ds.close_window()
        np.testing.assert_array_equal(ds.dense().astype(np.int64), want)
        assert ds.stats() == (int((want >= 0).sum()), 1)
        assert ds.checksum()[0] == dense_checksum(want)[0]
        probe = np.array([cap - 1, cap, -1, 0], dtype=np.int64)
        if bits == 32:                                   # (no negative ids in 32 bits: the invalid id)
            probe = np.array([cap - 1, cap, 0xFFFFFFFF, 0], dtype=np.uint32)
        assert ds.find_batch(probe).tolist() == [int(want[cap - 1]), -1, -1, 0]
        ds.reset()
        assert ds.stats() == (0, 0)
    ds.close()
