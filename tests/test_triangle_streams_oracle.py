"""CPU: the sparse-product triangle reference (tests/triangle_streams.py) equals the older oracles
and every closed form, and each structured family meets the input condition it exists for (id
bits, edge counts past one grid trip, long-row counts, row lengths at the tile edges)."""
import numpy as np
import pytest

import triangle_streams as ts
from triangles_oracle import dense_count, drop_self_loops, literal_window_count, random_multigraph


@pytest.mark.parametrize("nv,n", [(8, 40), (64, 600), (300, 6000)])
def test_sparse_count_equals_dense_and_literal(nv, n):
    src, dst = random_multigraph(nv, n, seed=nv + n)
    assert np.any(src == dst)
    total, ids, local, m = ts.sparse_count(src, dst)
    want_total, want_local = dense_count(src, dst, nv)
    assert total == want_total == literal_window_count(*drop_self_loops(src, dst)) > 0
    np.testing.assert_array_equal(ts.scatter_local(ids, local, nv), want_local)
    assert int(local.sum()) == 3 * total
    pairs = set(zip(np.minimum(src, dst).tolist(), np.maximum(src, dst).tolist())) - {(v, v) for v in range(nv)}
    assert m == len(pairs)
    assert set(ids.tolist()) == {x for p in pairs for x in p}


@pytest.mark.parametrize("nv,n", [(8, 40), (64, 600), (300, 6000)])
def test_masked_gram_is_the_masked_product(nv, n):
    import scipy.sparse as sp
    src, dst = random_multigraph(nv, n, seed=nv + n)
    keep = src != dst
    lo, hi = np.minimum(src[keep], dst[keep]), np.maximum(src[keep], dst[keep])
    U = sp.csr_matrix((np.ones(lo.size, dtype=np.int64), (lo, hi)), shape=(nv, nv))
    U.data[:] = 1                                                      # (repeated edges were summed)
    want = (U.T @ U).multiply(U)
    for chunk, direct in ((7, False), (1 << 18, False), (1 << 18, True), (1 << 18, None)):
        got = ts.masked_gram(U, chunk, direct)
        assert (got != want).nnz == 0 and got.sum() == want.sum() > 0


def test_sparse_count_edge_cases_and_known_answer():
    assert ts.sparse_count([], [])[0] == 0 and ts.sparse_count([], [])[3] == 0
    assert ts.sparse_count([5, 5], [5, 5]) [0] == 0
    total, ids, local, m = ts.sparse_count([9, 2, 7, 2, 9], [2, 7, 9, 9, 9])      # one triangle, a repeat, a loop
    assert (total, ids.tolist(), local.tolist(), m) == (1, [2, 7, 9], [1, 1, 1], 3)
    for src, dst, count in ts.known_answer():
        assert ts.sparse_count(src, dst)[0] == count
    assert [c for _, _, c in ts.known_answer()] == [2, 3, 2]
    assert sum(s.size for s, _, _ in ts.known_answer()) == 19


def test_bits_for():
    assert [ts.bits_for(c) for c in (1, 2, 3, 64, 65, 45000, 1 << 16, (1 << 16) + 1, ts.WIDE_CAPACITY)] \
        == [1, 1, 2, 6, 7, 16, 16, 17, 21]


def test_wide_grid():
    src, dst, cap, ident = ts.wide_grid()
    total, full, m = ts.reference("wide_grid")
    assert cap == (1 << 20) + 3 and ts.bits_for(cap) == 21
    assert 2 * ts.bits_for(cap) > 32                                   # keys need more than 32 bits
    assert src.size == ts.WIDE_GRID_SIMPLE + (1 << 18) + 1000 and src.size > ts.GRID_SPAN
    assert m == ts.WIDE_GRID_SIMPLE == 1077601 and m > 1048576 == ts.GRID_SPAN
    assert total == ts.wide_grid_total() == 717602
    assert np.unique(ident).size == ident.size == 360000               # an injection
    assert ident.min() == 0 and ident.max() == cap - 1
    assert {0, cap - 1} <= set(src.tolist()) | set(dst.tolist())
    assert int(np.sum(src == dst)) == 1000
    assert 0.45 < np.mean(src < dst) < 0.55                            # about half reversed
    assert int(full.sum()) == 3 * total
    grid = full[ident].reshape(ts.GRID_R, ts.GRID_C)
    assert np.all(grid[1:-1, 1:-1] == 6)
    assert grid[0, 0] == grid[-1, -1] == 2 and grid[0, -1] == grid[-1, 0] == 1
    assert np.all(grid[0, 1:-1] == 3) and np.all(grid[1:-1, 0] == 3)
    assert np.count_nonzero(full) == 360000                            # every other entry is 0
    # a key is a << 21 | b: any smaller end a >= 2^11 puts it past 2^32
    assert int(np.minimum(src, dst).max()) >= 1 << 11


def test_many_long_rows():
    src, dst, cap = ts.many_long_rows()
    total, full, m = ts.reference("many_long_rows")
    assert cap == 4330 and src.size == m == 4200 * 66 + 130 * 129 // 2
    assert total == ts.many_long_rows_total() == 4200 * (66 * 65 // 2) + 130 * 129 * 128 // 6 == 9366760
    assert int(full.sum()) == 3 * total
    assert src.size >= 266240 and src.size // (ts.KSHORT + 1) + 1 >= ts.MAX_BLOCKS    # the long-row grid is at its cap
    for by_degree in (True, False):
        rows = ts.out_row_lengths(src, dst, cap, by_degree)
        assert int(rows.sum()) == m
        assert int(np.sum(rows > ts.KSHORT)) > ts.MAX_BLOCKS          # a workgroup serves a second row
        assert np.all(rows[:4200] == 66)
    assert np.all(full[:4200] == 66 * 65 // 2)


@pytest.mark.parametrize("L", ts.TILE_SIZES)
def test_tile_edges(L):
    src, dst, cap = ts.tile_edges(L)
    total, full, m = ts.reference("tile_edges", L)
    assert cap == L + 1 and m == src.size == L + (L - 1) + max(L - 8193, 0)
    assert total == ts.tile_edges_total(L) == (L - 1) + max(L - 8193, 0)
    assert full[0] == total and int(full.sum()) == 3 * total
    rows = ts.out_row_lengths(src, dst, cap, by_degree=False)
    assert rows[0] == L and rows[1:].max() <= 2                        # one long row: the hub's
    assert ts.out_row_lengths(src, dst, cap, by_degree=True).max() <= ts.KSHORT
    assert ts.TILE_SIZES == (8191, 8192, 8193, 16384, 16385)


@pytest.mark.parametrize("with_clique", [False, True])
def test_regular_long(with_clique):
    src, dst, cap = ts.regular_long(with_clique)
    total, full, m = ts.reference("regular_long", with_clique)
    assert cap == 4099 + (200 if with_clique else 0)
    assert m == src.size == 4099 * 80 + (199 * 100 if with_clique else 0)
    assert total == ts.regular_long_total(with_clique) == 4099 * 3160 + (1313400 if with_clique else 0)
    assert np.all(full[:4099] == 3 * 3160) and np.all(full[4099:] == 19701)
    deg = np.bincount(np.concatenate([src, dst]), minlength=cap)
    assert np.all(deg[:4099] == 160)
    rows = ts.out_row_lengths(src, dst, cap, by_degree=True)
    np.testing.assert_array_equal(rows[:4099], ts.out_row_lengths(src, dst, cap, by_degree=False)[:4099])
    assert rows.max() == (199 if with_clique else 160) and rows[0] == 160
    assert int(np.sum(rows > ts.KSHORT)) > 4000                        # long rows under the degree orientation


def test_wide_windows():
    src, dst, cap, W = ts.wide_windows()
    ref = ts.window_reference()
    gs = ts.wide_grid()[0]
    assert W == 1 << 18 and cap == ts.WIDE_CAPACITY
    full = -(-gs.size // W)
    assert len(ref) == full + 2 == -(-src.size // W) == 8
    np.testing.assert_array_equal(src[:gs.size], gs)
    assert all(t > 0 and m > 0 for t, m in ref[:full])
    assert ref[full] == (0, 0)                                         # self-loops only
    lo = (full + 1) * W
    assert np.all(src[full * W:lo] == dst[full * W:lo])
    assert ref[full + 1] == (0, 2999) and src.size - lo == 2999        # the path
    assert {0, cap - 1} <= set(src[lo:].tolist()) | set(dst[lo:].tolist())
    whole = ts.sparse_count(src, dst)
    assert whole[0] == ts.wide_grid_total() and sum(t for t, _ in ref) < whole[0]
