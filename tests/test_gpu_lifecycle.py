"""GPU: the life of a handle's resources (csrc/owned.hpp): every lazily created group in one handle,
before and after a reset; buffers that regrow while work is queued; handles created and destroyed
in numbers. Every result is compared with oracle/pyoracle.py; every call must return GS_OK (the
bindings raise otherwise) unless the test says which error it expects."""
import json
import os
import threading

import numpy as np
import pytest

from gsgpu import DisjointSet, _abi
from gsgpu._abi import GsError
from gsgpu.bipartite import Candidates
from gsgpu.comm import Comm
from pyoracle import PyDisjointSet

pytestmark = pytest.mark.gpu

N = 1 << 12                  # edges, over ids < CAP
CAP = 1 << 12


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def edges():
    """The seeded random stream, read only: (src, dst) int64, and the oracle's canonical labels
    after n edges (dense array, -1 = not in the summary)."""
    rng = np.random.default_rng(20)
    s, d = rng.integers(0, CAP, N), rng.integers(0, CAP, N)
    memo = {}

    def labels(n):
        if n not in memo:
            o = PyDisjointSet()
            for a, b in zip(s[:n].tolist(), d[:n].tolist()):
                o.union(a, b)
            lab = np.full(CAP, -1, dtype=np.int64)
            for v, r in o.canonical().items():
                lab[v] = r
            memo[n] = lab
        return memo[n]
    return s, d, labels


def _text(s, d):
    return b"".join(b"%d %d\n" % (a, b) for a, b in zip(s.tolist(), d.tolist()))


def _check_pairs(v, l, want, ids=None):
    """(v, l) = every vertex of the summary with its label, sorted by vertex."""
    v, l = np.asarray(v).astype(np.int64), np.asarray(l).astype(np.int64)
    pv = np.nonzero(want >= 0)[0]
    pl = want[pv]
    if ids is not None:                              # sparse ids: slot numbers -> the ids the test used
        order = np.argsort(ids[pv])
        pv, pl = ids[pv][order], ids[pl][order]
    np.testing.assert_array_equal(v, pv)
    np.testing.assert_array_equal(l, pl)


@pytest.mark.parametrize("kind", ["dense32", "dense64", "sparse"])
def test_every_lazy_group_in_one_handle_before_and_after_reset(torch_cuda, edges, kind):
    torch = torch_cuda
    s, d, labels = edges
    bits = 32 if kind == "dense32" else 64
    sparse = kind == "sparse"
    npdt, tdt = (np.int32, torch.int32) if bits == 32 else (np.int64, torch.int64)
    # sparse ids: an increasing map of the stream's ids onto any longs (the minimum stays the minimum)
    ids = np.sort(np.random.default_rng(21).integers(-(1 << 62), 1 << 62, CAP)) if sparse else None
    hs, hd = (ids[s], ids[d]) if sparse else (s.astype(npdt), d.astype(npdt))
    half = N // 2
    ds = DisjointSet(CAP, id_bits=bits, sparse=sparse, staging_edges=1000)     # (several staging chunks)
    results = []
    for _ in range(2):
        out = []
        ds.fold(hs[:half], hd[:half])                # host buffers: the staging stream and its events
        want = labels(half)
        if not sparse:
            v, l = ds.delta()                        # pageable buffers, the whole emission
            _check_pairs(v, l, want)
            out.append((v.copy(), l.copy()))
            pin = [torch.empty(CAP, dtype=tdt).pin_memory() for _ in range(2)]
            ds.fold(hs[half:half + 512], hd[half:half + 512])
            ds.delta_async(*pin)                     # a pinned buffer: copied out on the emission stream
            ((v, l),) = ds.emit_wait(0)
            mirror = want.copy()
            mirror[v.numpy().astype(np.int64)] = l.numpy().astype(np.int64)
            np.testing.assert_array_equal(mirror, labels(half + 512))
            out.append((v.numpy().copy(), l.numpy().copy()))
            ds.fold(hs[half + 512:half + 1024], hd[half + 512:half + 1024])
            ds.delta_async(np.empty(CAP, dtype=npdt), np.empty(CAP, dtype=npdt))   # pageable: copied at the wait
            ((v, l),) = ds.emit_wait(0)
            mirror[v.astype(np.int64)] = l.astype(np.int64)
            np.testing.assert_array_equal(mirror, labels(half + 1024))
            out.append((v.copy(), l.copy()))
            done = half + 1024
            # the giant pre-filter over host edges: survivors are input edges, a dropped edge joins nothing
            want = labels(done)
            o = torch.full((2 * half,), -1, dtype=torch.int32, device="cuda")
            cnt = ds.filter_edges(hs[:half], hd[:half], o)
            rows = o.cpu().numpy().view(np.uint32).astype(np.int64).reshape(-1, 2)
            assert (rows[cnt:] == 0xFFFFFFFF).all()
            kin, cin = np.unique(s[:half] * CAP + d[:half], return_counts=True)
            kout, cout = np.unique(rows[:cnt, 0] * CAP + rows[:cnt, 1], return_counts=True)
            assert np.isin(kout, kin).all()
            kept = np.zeros(kin.size, dtype=np.int64)
            kept[np.searchsorted(kin, kout)] = cout
            assert (kept <= cin).all()
            dropped = kin[kept < cin]
            assert (want[dropped // CAP] == want[dropped % CAP]).all()
            out.append(np.sort(rows[:cnt, 0] * CAP + rows[:cnt, 1]))
        else:
            done = half
        v, l = ds.pairs()                            # emit_pairs with host buffers
        _check_pairs(v, l, labels(done), ids)
        out.append((v.copy(), l.copy()))
        q = np.arange(0, CAP, 3)
        lab, found = ds.find_batch_flags(ids[q] if sparse else q.astype(npdt))     # find_flags, host buffers
        want = labels(done)
        np.testing.assert_array_equal(found, want[q] >= 0)
        np.testing.assert_array_equal(lab[found], (ids[want[q]] if sparse else want[q])[found])
        n_e, n_w = ds.fold_text(_text(hs[done:], hd[done:]), 1000, chunk_bytes=1 << 12)   # the ingestion streams
        assert (n_e, n_w) == (N - done, -(-(N - done) // 1000))
        v, l = ds.pairs()
        _check_pairs(v, l, labels(N), ids)
        out.append((v.copy(), l.copy()))
        results.append(out)
        ds.reset()
    for a, b in zip(*results):                       # the same sequence after reset: the same results
        for x, y in zip(a, b) if isinstance(a, tuple) else [(a, b)]:
            np.testing.assert_array_equal(x, y)
    ds.close()


def test_buffers_regrow_while_work_is_queued(torch_cuda, edges):
    torch = torch_cuda
    s, d, labels = edges
    s32, d32 = s.astype(np.int32), d.astype(np.int32)
    want = labels(N)
    ds = DisjointSet(CAP, id_bits=32)
    ds.fold(torch.from_numpy(s32).cuda(), torch.from_numpy(d32).cuda())
    for n in (64, 1 << 14):                          # find: the emission temporaries grow
        q = (np.arange(n) * 7 % CAP).astype(np.int32)
        np.testing.assert_array_equal(ds.find_batch(q), want[q])
    for n in (1 << 10, 1 << 14):                     # filter_edges: its scratch and its staging grow
        a, b = np.resize(s32, n), np.resize(d32, n)
        o = torch.full((2 * n,), -1, dtype=torch.int32, device="cuda")
        cnt = ds.filter_edges(a, b, o)
        rows = o.cpu().numpy().view(np.uint32).astype(np.int64).reshape(-1, 2)
        assert (rows[cnt:] == 0xFFFFFFFF).all()
        # a survivor is an input edge, no more often than the input has it
        kin, cin = np.unique(a.astype(np.int64) * CAP + b, return_counts=True)
        kout, cout = np.unique(rows[:cnt, 0] * CAP + rows[:cnt, 1], return_counts=True)
        assert np.isin(kout, kin).all() and (cout <= cin[np.searchsorted(kin, kout)]).all()
    small = [torch.empty(16, dtype=torch.int32).pin_memory() for _ in range(2)]
    ds.delta_async(*small)                           # a slot of 16 pairs: too small, nothing consumed
    with pytest.raises(GsError) as e:
        ds.emit_wait(0)
    assert e.value.code == _abi.GS_ERR_CAPACITY
    full = [torch.empty(CAP, dtype=torch.int32).pin_memory() for _ in range(2)]
    ds.delta_async(*full)                            # the slot regrown: the whole emission
    ((v, l),) = ds.emit_wait(0)
    _check_pairs(v.numpy(), l.numpy(), want)
    text = _text(s, d)
    for chunk in (1 << 12, 1 << 15):                 # fold_text: the staging and the edge ring grow
        ds.reset()
        assert ds.fold_text(text, 512, chunk_bytes=chunk) == (N, N // 512)
        np.testing.assert_array_equal(ds.dense().astype(np.int64), want)
    ds.close()


def test_handle_churn(torch_cuda, edges):
    torch = torch_cuda
    s, d, labels = edges
    cap, n = 1 << 10, 256
    hs, hd = (s[:n] % cap).astype(np.int32), (d[:n] % cap).astype(np.int32)    # one small stream
    o = PyDisjointSet()
    for a, b in zip(hs.tolist(), hd.tolist()):
        o.union(a, b)
    want = np.full(cap, -1, dtype=np.int64)
    for v, r in o.canonical().items():
        want[v] = r
    alive = []
    for i in range(64):                              # 64 handles, 8 alive at once
        ds = DisjointSet(cap, id_bits=32, track_marks=bool(i & 1))
        if i & 2:
            ds.fold(hs, hd)
        else:
            ds.fold(torch.from_numpy(hs).cuda(), torch.from_numpy(hd).cuda())
        alive.append(ds)
        if len(alive) == 8:
            old = alive.pop(0)
            np.testing.assert_array_equal(old.dense().astype(np.int64), want)
            old.close()
    for ds in alive:
        np.testing.assert_array_equal(ds.dense().astype(np.int64), want)
        ds.close()
    # bipartiteness summaries, both engines, on the reference's two known-answer streams
    from pyoracle import coracle
    kat = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_kats.json")))["BipartitenessCheckTest"]
    for literal in (False, True):
        for which in ("bipartite", "non_bipartite"):
            e = np.array(kat[which + "_edges"], dtype=np.int64)
            a, b = np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1])
            c = Candidates(int(e.max()) + 1, id_bits=64, literal=literal)
            c.fold(a, b)
            c.close_window()
            assert c.status()[0] == coracle().bip_run(a, b, a.size)[0] == (which == "bipartite")
            c.close()
    # a 2-rank in-process communicator, one window exchanged
    comms = Comm.local_group(2, 0)
    errors, finals = [], [None, None]

    def rank(r):
        try:
            ds = DisjointSet(cap, id_bits=32, track_marks=True)
            lo, hi = r * n // 2, (r + 1) * n // 2
            ds.fold(hs[lo:hi], hd[lo:hi])
            ds.merge_window(comms[r], "allgather")
            finals[r] = ds.dense().astype(np.int64)
            ds.close()
        except Exception as e:                       # reported below
            errors.append((r, repr(e)))
    th = [threading.Thread(target=rank, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=60)
    assert not any(t.is_alive() for t in th) and not errors, errors
    for c in comms:
        c.close()
    for r in range(2):
        np.testing.assert_array_equal(finals[r], want)
