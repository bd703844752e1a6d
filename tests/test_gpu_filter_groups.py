"""k_filter_out's group loader at its boundaries (DisjointSet.filter_edges, csrc/cc_kernels.hpp):
whole groups of 4 edges load as 16-byte vectors when both streams are 16-byte aligned; an unaligned
stream and the ragged last group of any stream load by element. Both paths must keep the same edges.

A summary of capacity 2^12 folds and closes one 2^14-edge RMAT-12 window (a giant and its bitmap
exist), then filters slices of the stream's next edges: n = 1, 3 (a partial group alone), 4 (one
whole group), 63, 65 (whole groups, then 3 edges / 1 edge), 257 (one wave's 64 groups, then 1 edge)
and 4099 (one workgroup's 1024 groups, then 3 edges for a second workgroup). At this size the handle
has no hot set, so an edge is dropped iff both endpoints' giant bits are set: the survivors are
deterministic.
"""
import numpy as np
import pytest

from gsgpu import DisjointSet, GsError, _abi

pytestmark = pytest.mark.gpu

SCALE, CAP, WINDOW, SEED = 12, 1 << 12, 1 << 14, 32
SIZES = [1, 3, 4, 63, 65, 257, 4099]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def stream(oracle):
    """The window that is folded, and the slice that is filtered (the stream's next edges)."""
    s, d = oracle.gen_rmat(0, WINDOW, SCALE, SEED)
    s2, d2 = oracle.gen_rmat(WINDOW, max(SIZES), SCALE, SEED)
    return s, d, s2, d2


@pytest.fixture(scope="module", params=[32, 64])
def summary(request, torch_cuda, stream):
    """(ds, labels): the closed summary and its dense labels, shared and only read by the tests."""
    torch = torch_cuda
    dt = torch.int32 if request.param == 32 else torch.int64
    ds = DisjointSet(CAP, id_bits=request.param, stream=torch.cuda.current_stream())
    ds.fold(torch.from_numpy(stream[0]).to(dt).cuda(), torch.from_numpy(stream[1]).to(dt).cuda())
    ds.close_window()
    labels = ds.dense().astype(np.int64)
    yield ds, labels
    ds.close()


def _device_pair(torch, ds, s, d, aligned):
    """s, d as device tensors of the handle's id width: fresh allocations (16-byte aligned), or views
    that start one element into a larger tensor (4 or 8 bytes past a 16-byte boundary)."""
    dt = torch.int32 if ds.id_bits == 32 else torch.int64
    out = []
    for a in (s, d):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dt)
        if aligned:
            t = t.cuda()
        else:
            big = torch.zeros(t.numel() + 5, dtype=dt, device="cuda")
            big[1:1 + t.numel()] = t.cuda()
            t = big[1:1 + t.numel()]
        assert (t.data_ptr() % 16 == 0) == aligned
        out.append(t)
    return out


def _filter(torch, ds, s, d, aligned):
    """The survivors of (s, d) as sorted keys u * CAP + v, and the raw (u, v) rows written."""
    ts, td = _device_pair(torch, ds, s, d, aligned)
    out = torch.full((2 * len(s),), -1, dtype=torch.int32, device="cuda")
    try:
        cnt = ds.filter_edges(ts, td, out)
        err = None
    except GsError as e:
        cnt, err = None, e.code
    rows = out.cpu().numpy().view(np.uint32).astype(np.int64).reshape(-1, 2)
    if cnt is None:                                   # the rows written before the error: not the fill value
        rows = rows[(rows != 0xFFFFFFFF).any(axis=1)]
    else:
        assert (rows[cnt:] == 0xFFFFFFFF).all(), "rows written past the returned count"
        rows = rows[:cnt]
    return np.sort(rows[:, 0] * CAP + rows[:, 1]), rows, err


@pytest.mark.parametrize("n", SIZES)
def test_aligned_and_element_loads_keep_the_same_edges(torch_cuda, stream, summary, n):
    ds, labels = summary
    s, d = stream[2][:n], stream[3][:n]
    ka, ra, ea = _filter(torch_cuda, ds, s, d, aligned=True)
    ku, ru, eu = _filter(torch_cuda, ds, s, d, aligned=False)
    print("n=%d id_bits=%d: %d survivors aligned, %d unaligned" % (n, ds.id_bits, ka.size, ku.size))
    assert ea is None and eu is None
    np.testing.assert_array_equal(ka, ku)             # the same survivor multiset from both loaders
    # a sub-multiset of the input: no key more often than the input has it
    kin, cin = np.unique(s * CAP + d, return_counts=True)
    kout, cout = np.unique(ka, return_counts=True)
    assert ra.size == 0 or (ra.max() < CAP)
    assert np.isin(kout, kin).all()
    kept = np.zeros(kin.size, dtype=np.int64)
    kept[np.searchsorted(kin, kout)] = cout
    assert (kept <= cin).all()
    # every dropped edge joins two vertices of one component (both seen, equal labels)
    dropped = np.repeat(kin, cin - kept)
    du, dv = dropped // CAP, dropped % CAP
    assert (labels[du] >= 0).all() and (labels[du] == labels[dv]).all()
    if n == max(SIZES):                               # not vacuous: the filter both drops and keeps
        assert dropped.size >= 1 and ka.size >= 1


@pytest.mark.parametrize("aligned", [True, False])
def test_out_of_range_id_in_the_ragged_last_group(torch_cuda, stream, summary, aligned):
    """An id >= capacity in the last, partial group (edges 4096..4098 of 4099): the call raises
    GS_ERR_RANGE, the edge is not among the rows written, and the other edges' survivors are."""
    ds, _ = summary
    n = max(SIZES)
    s, d = stream[2][:n].copy(), stream[3][:n].copy()
    good, _, err = _filter(torch_cuda, ds, s[:n - 1], d[:n - 1], aligned)
    assert err is None
    s[n - 1] = CAP                                    # the smallest id out of range
    keys, rows, err = _filter(torch_cuda, ds, s, d, aligned)
    assert err == _abi.GS_ERR_RANGE
    assert rows.size == 0 or rows.max() < CAP         # the bad edge was not returned
    np.testing.assert_array_equal(keys, good)         # (nor anything in its place)
