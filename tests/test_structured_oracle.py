"""The structured streams of tests/structured_streams.py on the CPU: the C oracle's per-window
checksums and final labels against scipy's connected components (canonical label = the minimum id
of the component), every window of every family; and the properties the families exist for, as
conditions on the inputs computed from scipy's labels (tests/test_gpu_structured.py folds the same
streams on the GPU and relies on them: a giant that is a comb, many mature windows without one, ...).
"""
import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import structured_streams as ss
from pyoracle import dense_checksum

N, W = ss.N, ss.W


def _canonical(src, dst, seen):
    """Min-id labels of the graph (src, dst) over N vertices; -1 where not seen."""
    g = coo_matrix((np.ones(src.size, dtype=np.int8), (src, dst)), shape=(N, N)).tocsr()
    nc, comp = connected_components(g, directed=False)
    mins = np.empty(nc, dtype=np.int64)
    ids = np.arange(N, dtype=np.int64)
    mins[comp[::-1]] = ids[::-1]                         # the last store is the smallest id
    lab = mins[comp]
    lab[~seen] = -1
    return lab


def _window_stats(name):
    """Per window of W edges: scipy's labels of the prefix (each window's graph: the labels so far
    as edges (v, label) plus the window's edges), reduced to what the tests need."""
    s, d = ss.stream(name)
    seen = np.zeros(N, dtype=bool)
    lab = np.full(N, -1, dtype=np.int64)
    out = []
    for lo in range(0, s.size, W):
        ws, wd = s[lo:lo + W], d[lo:lo + W]
        st = {}
        if seen.any():                                   # the window's edges against the giant before it
            cnt = np.bincount(lab[seen])
            g = int(np.argmax(cnt))
            a, b = lab[ws] == g, lab[wd] == g
            st["both"], st["one"] = float(np.mean(a & b)), float(np.mean(a ^ b))
        v = np.nonzero(seen)[0]
        seen[ws] = True
        seen[wd] = True
        lab = _canonical(np.concatenate([v, ws]), np.concatenate([lab[v], wd]), seen)
        h, nv, nc = dense_checksum(lab)
        st.update(checksum=h, vertices=nv, components=nc, largest=int(np.bincount(lab[seen]).max()))
        out.append(st)
    return out, lab


_STATS = {}


def _stats(name):
    if name not in _STATS:
        _STATS[name] = _window_stats(name)
    return _STATS[name]


@pytest.mark.parametrize("name", ss.FAMILIES)
def test_oracle_equals_scipy_every_window(oracle, name):
    stats, final = _stats(name)
    want = ss.oracle_windows(oracle, name)
    assert [int(x) for x in want["checksums"]] == [st["checksum"] for st in stats]
    assert [tuple(int(x) for x in c) for c in want["counts"]] == [(st["vertices"], st["components"]) for st in stats]
    np.testing.assert_array_equal(want["final"], final)
    s, d = ss.stream(name)                               # and scipy on the whole stream at once
    seen = np.zeros(N, dtype=bool)
    seen[s] = True
    seen[d] = True
    np.testing.assert_array_equal(final, _canonical(s, d, seen))


@pytest.mark.parametrize("name", ss.FAMILIES)
def test_oracle_window_2_19(oracle, name):
    """The oracle in windows of 2^19 edges: every window that ends where one of 2^16 does has that
    window's checksum."""
    stats, final = _stats(name)
    want = ss.oracle_windows(oracle, name, 1 << 19)
    nwin = len(stats)
    ends = [min(8 * (k + 1), nwin) - 1 for k in range(len(want["checksums"]))]
    assert len(ends) == -(-nwin // 8)
    assert [int(x) for x in want["checksums"]] == [stats[e]["checksum"] for e in ends]
    np.testing.assert_array_equal(want["final"], final)


def test_comb_is_a_comb():
    stats, final = _stats("comb")
    assert len(stats) == 16
    for w in range(ss.COMB_SPINE_WINDOWS - 1, len(stats)):        # from the close of window 4 on
        assert stats[w]["largest"] >= 0.70 * stats[w]["vertices"], w
    for w in ss.comb_mix_windows():
        assert stats[w]["both"] >= 0.40 and stats[w]["one"] >= 0.20, (w, stats[w])
    assert final[ss.SPINE_LO] == 0 and final[N - 1] == 0 and final[N - 2] == 0 and final[N - 3] == 0
    assert stats[-1]["components"] == 1
    # the outside chains are outside until the attach windows
    assert stats[ss.COMB_SPINE_WINDOWS + ss.COMB_MIX_WINDOWS - 1]["components"] > 18000
    assert stats[ss.COMB_SPINE_WINDOWS + ss.COMB_MIX_WINDOWS + ss.COMB_ATTACH_WINDOWS - 1]["components"] == 1


def test_equal_paths_have_no_giant():
    stats, final = _stats("equal_paths")
    assert len(stats) == ss.EQ_GROW_WINDOWS + ss.EQ_JOIN_WINDOWS
    for w in range(ss.EQ_GROW_WINDOWS):
        assert 4 * stats[w]["largest"] < stats[w]["vertices"], w
    assert stats[ss.EQ_GROW_WINDOWS - 1]["components"] == 16
    assert [st["components"] for st in stats[ss.EQ_GROW_WINDOWS:]] == [8, 4, 2, 1]
    assert 4 * stats[ss.EQ_GROW_WINDOWS]["largest"] < stats[ss.EQ_GROW_WINDOWS]["vertices"]    # 16 -> 8: still none
    assert final[ss.EQ_LO] == ss.EQ_LO


@pytest.mark.parametrize("name", ["shuffled_path", "bitrev_path"])
def test_scattered_paths_have_no_giant_for_half_the_stream(name):
    stats, _ = _stats(name)
    for w in range((len(stats) + 1) // 2):
        assert 4 * stats[w]["largest"] < stats[w]["vertices"], w
    assert stats[-1]["components"] == 1 and stats[-1]["vertices"] == N


def test_matching_components():
    stats, _ = _stats("matching")
    m = ss.matching_windows()
    assert stats[m - 1]["components"] == N // 2 and stats[m - 1]["largest"] == 2
    assert all(st["largest"] == 2 for st in stats[:m])
    assert stats[-1]["components"] == 1 and stats[-1]["vertices"] == N


@pytest.mark.parametrize("name", ["asc_path", "desc_path", "star_max_hub", "binary_tree_desc"])
def test_single_component_families(name):
    stats, final = _stats(name)
    assert stats[-1]["components"] == 1 and stats[-1]["vertices"] == N
    assert all(st["components"] == 1 for st in stats)          # one growing tree: a giant from window 1


@pytest.mark.parametrize("cap", ss.ODD_CAPS)
def test_odd_capacity_expectation(cap):
    s, d, lab, windows = ss.odd_capacity_stream(cap)
    assert max(s.max(), d.max()) == cap - 1 or cap == 1
    assert lab.size == cap and len(windows) == 3 and windows[0][0] == 0 and windows[-1][1] == s.size
    assert all(a[1] == b[0] for a, b in zip(windows, windows[1:]))
    seen = np.zeros(cap, dtype=bool)
    seen[s] = True
    seen[d] = True
    g = coo_matrix((np.ones(s.size, dtype=np.int8), (s, d)), shape=(cap, cap)).tocsr()
    nc, comp = connected_components(g, directed=False)
    mins = np.empty(nc, dtype=np.int64)
    mins[comp[::-1]] = np.arange(cap, dtype=np.int64)[::-1]
    want = mins[comp]
    want[~seen] = -1
    np.testing.assert_array_equal(lab, want)
