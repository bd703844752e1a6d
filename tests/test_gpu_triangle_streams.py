"""GPU parity of the triangle counter (gs_tri_*) on the structured families of
tests/triangle_streams.py against its sparse-product reference: keys wider than 32 bits, windows
of more than one grid trip, more long rows than long-row workgroups, rows at the LDS tile's edges,
long rows under the degree orientation, and one handle across all of them. Integer path: every
comparison is exact."""
import ctypes

import numpy as np
import pytest

import triangle_streams as ts
from gsgpu import GsError, TriangleCounter
from gsgpu import _abi

pytestmark = pytest.mark.gpu

ORIENTS = ["degree", "id"]
ONE_WINDOW = ([("many_long_rows", None)] + [("tile_edges", L) for L in ts.TILE_SIZES]
              + [("regular_long", False), ("regular_long", True)])
U64 = ctypes.c_uint64


def _family(name, arg):
    return (ts.FAMILIES[name](arg) if arg is not None else ts.FAMILIES[name]())[:3]


def _check_local(tc, src, dst, total, full, m):
    """count_local: the total, every entry of the capacity-long array (the reference's counts at
    its ids, 0 everywhere else) and the simple-edge count."""
    got_total, got_local, got_m = tc._local(src, dst, True)
    assert got_total == total and got_m == m
    assert got_local.shape == full.shape
    np.testing.assert_array_equal(got_local, full)


@pytest.mark.parametrize("orient", ORIENTS)
@pytest.mark.parametrize("id_bits", [32, 64])
@pytest.mark.parametrize("name,arg", ONE_WINDOW)
def test_family_equals_the_reference(name, arg, id_bits, orient):
    src, dst, cap = _family(name, arg)
    total, full, m = ts.reference(name, arg)
    with TriangleCounter(cap, id_bits=id_bits, orient=orient) as tc:
        assert tc.count(src, dst) == total
        assert tc.count_windows(src, dst, src.size).tolist() == [total]
        assert tc.simple_edges(src, dst) == m
        _check_local(tc, src, dst, total, full, m)


@pytest.mark.parametrize("orient", ORIENTS)
@pytest.mark.parametrize("id_bits", [32, 64])
def test_wide_grid_counts(id_bits, orient):
    src, dst, cap, _ = ts.wide_grid()
    total, full, m = ts.reference("wide_grid")
    with TriangleCounter(cap, id_bits=id_bits, orient=orient) as tc:
        assert tc.count(src, dst) == total == 717602
        assert tc.simple_edges(src, dst) == m == 1077601
        assert tc.count_windows(src, dst, src.size).tolist() == [total]
        if id_bits == 64:
            _check_local(tc, src, dst, total, full, m)


@pytest.mark.parametrize("orient", ORIENTS)
@pytest.mark.parametrize("id_bits", [32, 64])
def test_wide_grid_from_device_tensors(id_bits, orient):
    import torch
    src, dst, cap, _ = ts.wide_grid()
    total, full, m = ts.reference("wide_grid")
    dt = torch.int32 if id_bits == 32 else torch.int64
    s = torch.from_numpy(src.copy()).to("cuda").to(dt).contiguous()
    d = torch.from_numpy(dst.copy()).to("cuda").to(dt).contiguous()
    with TriangleCounter(cap, id_bits=id_bits, orient=orient) as tc:
        assert tc.count(s, d) == total
        assert tc.count_windows(s, d, ts.WIDE_SPLIT).tolist() == list(ts.wide_grid_split_reference())
        if id_bits == 32:
            _check_local(tc, s, d, total, full, m)


@pytest.mark.parametrize("orient", ORIENTS)
@pytest.mark.parametrize("id_bits", [32, 64])
def test_wide_windows(id_bits, orient):
    """Windows of 2^18 edges over 21-bit ids, a window of self-loops only, a path: the per-vertex
    row words must be clean again after every window."""
    src, dst, cap, W = ts.wide_windows()
    ref = ts.window_reference()
    with TriangleCounter(cap, id_bits=id_bits, orient=orient) as tc:
        assert tc.count_windows(src, dst, W).tolist() == [t for t, _ in ref]
        if id_bits == 32:
            for k, (t, m) in enumerate(ref):
                got_t, _, got_m = tc._local(src[k * W:(k + 1) * W], dst[k * W:(k + 1) * W], False)
                assert (got_t, got_m) == (t, m), k
        assert tc.count_windows(src, dst, W).tolist() == [t for t, _ in ref]


@pytest.mark.parametrize("orient", ORIENTS)
def test_one_handle_across_families(orient):
    """A small window, the widest one, the 19-edge known answer, then the long rows, on one handle
    (twice): the scratch grows once and is reused by smaller windows, and no per-vertex word of a
    window survives into the next."""
    cap = ts.WIDE_CAPACITY
    steps = [("tile_edges", ts.TILE_SIZES[0]), ("wide_grid", None), None, ("many_long_rows", None)]
    with TriangleCounter(cap, orient=orient) as tc:
        for again in range(2):
            for step in steps:
                if step is None:
                    for s, d, count in ts.known_answer():
                        assert tc.count(s, d) == count
                        total, local = tc.local(s, d)
                        assert total == count and int(local.sum()) == 3 * count
                        assert set(np.nonzero(local)[0].tolist()) <= set(s.tolist()) | set(d.tolist())
                    continue
                src, dst, small = _family(*step)
                total, full, m = ts.reference(*step)
                assert tc.count(src, dst) == total
                padded = np.zeros(cap, dtype=np.uint64)
                padded[:small] = full
                _check_local(tc, src, dst, total, padded, m)


@pytest.mark.parametrize("orient", ORIENTS)
@pytest.mark.parametrize("name,arg", [("many_long_rows", None), ("regular_long", True)])
def test_device_local_buffer_through_the_abi(name, arg, orient):
    """gs_tri_count_local with ``local`` in device memory: the same array as through the host."""
    import torch
    src, dst, cap = _family(name, arg)
    total, full, m = ts.reference(name, arg)
    src = np.ascontiguousarray(src, dtype=np.int64)
    dst = np.ascontiguousarray(dst, dtype=np.int64)
    local = torch.full((cap,), 7, dtype=torch.int64, device="cuda")       # stale contents: the call zeroes them
    torch.cuda.synchronize()
    got, simple = U64(), U64()
    with TriangleCounter(cap, orient=orient) as tc:
        rc = _abi.lib().gs_tri_count_local(tc.handle, src.ctypes.data_as(ctypes.c_void_p), dst.ctypes.data_as(ctypes.c_void_p),
                                           src.size, ctypes.c_void_p(local.data_ptr()), ctypes.byref(got), ctypes.byref(simple))
        assert rc == _abi.GS_OK
        assert (got.value, simple.value) == (total, m)
        np.testing.assert_array_equal(local.cpu().numpy().astype(np.uint64), full)
        host_total, host_local = tc.local(src, dst)
    assert host_total == total
    np.testing.assert_array_equal(host_local, full)


@pytest.mark.parametrize("orient", ORIENTS)
@pytest.mark.parametrize("bad", [(1 << 32) + 5, 1 << 40])
def test_wide_int64_id_is_a_range_error_before_truncation(bad, orient):
    """At capacity 64 the low 32 bits of 2^32 + 5 and of 2^40 are valid ids: the range check has to
    see all 64 bits."""
    windows = ts.known_answer()
    s, d, count = windows[1]
    assert max(int(s.max()), int(d.max())) < 64 and (bad & 0xFFFFFFFF) < 64
    with TriangleCounter(64, id_bits=64, orient=orient) as tc:
        for col in (0, 1):
            x, y = s.copy(), d.copy()
            (x if col == 0 else y)[3] = bad
            with pytest.raises(GsError) as ei:
                tc.count(x, y)
            assert ei.value.code == _abi.GS_ERR_RANGE
            with pytest.raises(GsError) as ei:
                tc.count_windows(x, y, 4)
            assert ei.value.code == _abi.GS_ERR_RANGE
            with pytest.raises(GsError) as ei:
                tc.local(x, y)
            assert ei.value.code == _abi.GS_ERR_RANGE
            assert tc.count(s, d) == count                                 # the handle is as good as new
            total, local = tc.local(s, d)
            assert total == count and int(local.sum()) == 3 * count


def test_count_local_of_no_edges_zeroes_the_array():
    import torch
    cap = 1000
    mark = np.uint64(0xDEADBEEF)
    local = np.full(cap, mark, dtype=np.uint64)
    dlocal = torch.full((cap,), 7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    got, simple = U64(5), U64(5)
    with TriangleCounter(cap) as tc:
        src, dst, _ = ts.tile_edges(ts.TILE_SIZES[0])                     # something before it, within the capacity
        keep = (src < cap) & (dst < cap)
        assert tc.count(src[keep], dst[keep]) == ts.sparse_count(src[keep], dst[keep])[0] > 0
        for buf in (local.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(dlocal.data_ptr())):
            got.value = simple.value = 5
            assert _abi.lib().gs_tri_count_local(tc.handle, None, None, 0, buf, ctypes.byref(got), ctypes.byref(simple)) == _abi.GS_OK
            assert (got.value, simple.value) == (0, 0)
    assert not local.any()
    assert not dlocal.cpu().numpy().any()
