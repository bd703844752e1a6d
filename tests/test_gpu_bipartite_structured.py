"""GPU parity of the parity union-find (csrc/bip.hip) on structured graphs
(tests/bipartite_streams.py) at the odd capacity 2^18 + 3: after every window status(), pairs() and
checksum() equal the double-cover reference (which tests/test_bipartite_structured_oracle.py checks
against the oracle's union-find, its BFS and closed forms). Integer path: every comparison exact.

What the families reach that random planted-bipartite streams do not:
  paths, cycles          deep trees under the no-return atomicMin halving while other lanes hook; the
                         odd-cycle decision made by an arbitrary last edge with parities accumulated
                         over a long walk (odd_cycle, odd_cycle_mid), or by a path edge that closes
                         under a chord folded long before (chord_first)
  star, K(512, 512)      one contended root word: failed hooks that re-read and re-walk
  grid, hypercube        many redundant consistent constraints racing with the hooks
  matching_loops         2^17 + 3 components, repeated edges both ways round, self-loops
and the code paths no other test reaches: gs_bip_fold_pairs, the vector fold against the scalar one
and the n % 4 tail, a conflict that only the merge sees, a smaller-capacity merge source, deep
uncompressed merge inputs, k_bip_scan with two tiles per thread, gs_bip_emit_pairs into device
buffers and with cap < total, the young split at cap / 4 in {0, 1}, the host staging loop across
its 2^22-edge chunk, and the signs of the stream `bench.py --workload bip` times.
"""
import ctypes

import numpy as np
import pytest

import bipartite_streams as bs
from bipartite import ParityUnionFind, emission_string, literal_run
from gsgpu import BipartitenessCheck, Candidates, GsError, SimpleEdgeStream
from gsgpu import _abi

pytestmark = pytest.mark.gpu

U64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


_DEV = {}


def _device_stream(torch, name, bits):
    """The family as device tensors of the handle's id width (made once per module)."""
    if (name, bits) not in _DEV:
        st = bs.stream(name)
        dt = np.int32 if bits == 32 else np.int64
        _DEV[name, bits] = (torch.from_numpy(st.src.astype(dt)).cuda(), torch.from_numpy(st.dst.astype(dt)).cuda())
    return _DEV[name, bits]


def _check(c, ref, what=""):
    """The summary equals the reference state: status, the three emission arrays, the checksum. A
    failed state: not bipartite, nothing emitted, "(false,{})"."""
    if not ref.ok:
        assert c.status()[0] is False, what
        ok, v, k, s = c.snapshot()
        assert (ok, v.size, k.size, s.size) == (False, 0, 0, 0), what
        assert c.checksum()[1] is False, what
        assert c.getMap() == {} and c.toString() == "(false,{})", what
        return
    assert c.status() == ref.status, what
    v, k, s = c.pairs()
    rv, rk, rs = ref.pairs()
    assert np.array_equal(v, rv), what
    assert np.array_equal(k, rk), what
    assert np.array_equal(s, rs), what
    assert c.checksum() == (ref.checksum, True, ref.n_vertices, ref.n_components), what


def _assert_empty(c):
    assert c.status() == (True, 0, 0) and c.pairs()[0].size == 0 and c.toString() == "(true,{})"
    assert c.checksum() == (0, True, 0, 0)


def _ref_of(src, dst, cap):
    return bs.Ref(*bs.cover_reference(src, dst, cap), cap)


# ---- 1. window by window ----
@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", bs.FAMILIES)
def test_every_window(torch_cuda, name, bits):
    """Candidates.fold + close_window per window from device arrays, every window compared; reset,
    the empty summary, and the stream a second time on the same handle."""
    st = bs.stream(name)
    refs = bs.reference_windows(name)
    ts, td = _device_stream(torch_cuda, name, bits)
    c = Candidates(st.cap, id_bits=bits, stream=torch_cuda.cuda.current_stream())
    for rnd in range(2):
        for w, ref in enumerate(refs):
            lo = w * st.W
            c.fold(ts[lo:lo + st.W], td[lo:lo + st.W])
            c.close_window()
            _check(c, ref, "round %d window %d" % (rnd, w))
        assert refs[-1].ok == (name not in bs.FAILING)
        c.reset()
        _assert_empty(c)
    c.close()


# ---- 2. one call from device buffers: the vector fold, the scalar fold, the tail ----
ONE_CALL = ("shuffled_path", "odd_cycle", "complete_bipartite", "hypercube")


@pytest.mark.parametrize("kind", ["int32_aligned", "int32_offset", "int64"])
@pytest.mark.parametrize("name", ONE_CALL)
def test_one_call_from_device(torch_cuda, name, kind):
    """The whole stream in one fold. int32 as allocated is 16-byte aligned (k_bip_fold<.., VEC>);
    views from element offsets 1, 2, 3 are not (the scalar kernel); the stream less its last 0..3
    edges has n % 4 in {0, 1, 2, 3} (the tail group), the reference given the same prefix."""
    torch = torch_cuda
    st = bs.stream(name)
    n = st.src.size
    bits = 64 if kind == "int64" else 32
    ts, td = _device_stream(torch, name, bits)
    cases = {"int32_aligned": [(0, n - k) for k in range(4)], "int32_offset": [(o, n - o) for o in (1, 2, 3)],
             "int64": [(0, n), (1, n - 1)]}[kind]
    assert kind != "int32_aligned" or sorted(m % 4 for _, m in cases) == [0, 1, 2, 3]
    c = Candidates(st.cap, id_bits=bits, stream=torch.cuda.current_stream())
    for off, m in cases:
        big_s = torch.empty(n + 4, dtype=ts.dtype, device="cuda")
        big_d = torch.empty(n + 4, dtype=ts.dtype, device="cuda")
        vs, vd = big_s[off:off + m], big_d[off:off + m]
        vs.copy_(ts[:m])
        vd.copy_(td[:m])
        if bits == 32:
            assert (vs.data_ptr() % 16 == 0 and vd.data_ptr() % 16 == 0) == (off == 0)
        c.reset()
        c.fold(vs, vd)
        c.close_window()
        _check(c, bs.reference_prefix(name, m), "offset %d, %d edges" % (off, m))
    c.close()


# ---- 3. pair folds (gs_bip_fold_pairs: k_bip_fold<*, AOS>) ----
def _fold_pairs(c, ptr, n):
    _abi.call("gs_bip_fold_pairs", c.handle, ctypes.c_void_p(ptr), int(n))


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", ["shuffled_path", "matching_loops", "odd_cycle"])
def test_pair_folds_every_window(torch_cuda, name, bits):
    """Interleaved (u, v) buffers, uint32 and int64, from host memory and from device memory, window
    by window: the same result as the two-array fold."""
    torch = torch_cuda
    st = bs.stream(name)
    refs = bs.reference_windows(name)
    dt = np.uint32 if bits == 32 else np.int64
    host = np.ascontiguousarray(np.stack([st.src, st.dst], axis=1).astype(dt))          # (n, 2)
    dev = torch.from_numpy(host.view(np.int32 if bits == 32 else np.int64)).cuda()
    assert dev.is_contiguous() and dev.shape == host.shape
    row = 2 * host.itemsize
    c = Candidates(st.cap, id_bits=bits, stream=torch.cuda.current_stream())
    for where, base in (("host", host.ctypes.data), ("device", dev.data_ptr())):
        c.reset()
        for w, ref in enumerate(refs):
            lo, hi = w * st.W, min((w + 1) * st.W, st.src.size)
            _fold_pairs(c, base + lo * row, hi - lo)
            c.close_window()
            _check(c, ref, "%s window %d" % (where, w))
    c.close()


@pytest.mark.parametrize("bits", [32, 64])
def test_pair_fold_range_error(bits):
    dt = np.uint32 if bits == 32 else np.int64
    c = Candidates(16, id_bits=bits)
    pairs = np.array([[1, 2], [3, 16], [2, 5], [16, 16], [7, 7]], dtype=dt)
    _fold_pairs(c, pairs.ctypes.data, len(pairs))
    with pytest.raises(GsError) as e:
        c.sync()
    assert e.value.code == _abi.GS_ERR_RANGE
    c.sync()                                                        # reported once
    assert c.toString() == "(true,{1={1=(1,true), 2=(2,false), 5=(5,true)}, 7={7=(7,true)}})"
    if bits == 64:
        bad = np.array([[-1, 2]], dtype=np.int64)
        _fold_pairs(c, bad.ctypes.data, 1)
        with pytest.raises(GsError) as e:
            c.sync()
        assert e.value.code == _abi.GS_ERR_RANGE
    c.close()


# ---- 4. partials and merges (k_bip_merge) ----
@pytest.mark.parametrize("name", ["shuffled_path", "even_cycle", "odd_cycle_mid", "grid_diag", "star_max_hub"])
def test_reference_mode_partials(name):
    """Three fresh partials per window, merged in partition order, then the Merger's merge with the
    cumulative summary: k_bip_merge inputs that are deep and uncompressed."""
    st = bs.stream(name)
    refs = bs.reference_windows(name)
    op = BipartitenessCheck(1000, vertex_capacity=st.cap, mode="reference", parallelism=3, window_edges=st.W)
    seen = 0
    for w, c in enumerate(SimpleEdgeStream(st.src, st.dst).aggregate(op)):
        _check(c, refs[w], "window %d" % w)
        seen += 1
    assert seen == len(refs)


def _halves(name):
    st = bs.stream(name)
    h = st.src.size // 2
    return st, (st.src[:h], st.dst[:h]), (st.src[h:], st.dst[h:])


def test_merge_conflict_only_in_the_merge():
    """The two halves of odd_cycle's edge list are bipartite on their own (unions of paths); the
    odd cycle exists only across them."""
    st, first, second = _halves("odd_cycle")
    a, b = Candidates(st.cap), Candidates(st.cap)
    a.fold(*first)
    b.fold(*second)
    ra, rb = _ref_of(*first, st.cap), _ref_of(*second, st.cap)
    assert ra.ok and rb.ok
    _check(a, ra)
    _check(b, rb)
    b2 = Candidates(st.cap)
    b2.fold(*second)                                                # uncompressed: no close, no status
    assert a.merge(b2) is a
    _check(a, bs.reference_windows("odd_cycle")[-1])
    assert not a.getSuccess()
    _check(b, rb)
    _check(b2, rb)                                                  # the source is left as it was
    for x in (a, b, b2):
        x.close()


@pytest.mark.parametrize("order", ["a_into_b", "b_into_a"])
def test_merge_of_deep_halves(order):
    st, first, second = _halves("even_cycle")
    a, b = Candidates(st.cap, id_bits=32), Candidates(st.cap, id_bits=32)
    a.fold(*first)
    b.fold(*second)
    into, frm = (b, a) if order == "a_into_b" else (a, b)
    into.merge(frm)
    _check(into, bs.reference_windows("even_cycle")[-1])
    a.close()
    b.close()


def test_merge_smaller_capacity_source_and_empty():
    small = bs.stream("hypercube", bs.L_SMALL)                      # capacity 2^12
    big = bs.stream("shuffled_path")
    assert small.cap == 1 << 12 and big.cap == bs.NB
    m = 2 * big.W
    s, t = Candidates(small.cap), Candidates(big.cap)
    s.fold(small.src, small.dst)
    t.fold(big.src[:m], big.dst[:m])
    rs, rt = _ref_of(small.src, small.dst, small.cap), bs.reference_prefix("shuffled_path", m)
    with pytest.raises(GsError) as e:
        s.merge(t)                                                  # a larger source: refused
    assert e.value.code == _abi.GS_ERR_RANGE
    _check(s, rs)
    _check(t, rt)
    t.merge(s)
    _check(t, _ref_of(np.concatenate([big.src[:m], small.src]), np.concatenate([big.dst[:m], small.dst]), big.cap))
    _check(s, rs)
    empty, empty_small = Candidates(big.cap), Candidates(small.cap)
    s.merge(empty_small)                                            # from an empty summary: unchanged
    _check(s, rs)
    empty.merge(s)                                                  # into an empty summary
    _check(empty, _ref_of(small.src, small.dst, big.cap))
    for x in (s, t, empty, empty_small):
        x.close()


def test_merge_across_two_streams(torch_cuda):
    """Summaries on two torch streams: the merge orders itself after `from`'s folds, and `from`
    stays usable: more folded into it after the merge lands after the merge's reads."""
    torch = torch_cuda
    st, first, second = _halves("even_cycle")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a, b = Candidates(st.cap, stream=s1), Candidates(st.cap, stream=s2)
    a.fold(*first)
    b.fold(*second)
    a.merge(b)
    q = st.src.size // 4
    b.fold(st.src[:q], st.dst[:q])
    _check(a, bs.reference_windows("even_cycle")[-1])
    _check(b, _ref_of(np.concatenate([second[0], st.src[:q]]), np.concatenate([second[1], st.dst[:q]]), st.cap))
    a.close()
    b.close()


# ---- 5. emission at 1,026 tiles (two per scan thread, one vertex in the last) ----
EMIT_CAP = (1 << 22) + 4097
_EMIT = {}


def _emit_case():
    if not _EMIT:
        rng = np.random.default_rng(301)
        must = np.array([0, 4095, 4096, (1 << 22) - 1, 1 << 22, EMIT_CAP - 1], dtype=np.int64)
        ids = np.unique(np.concatenate([must, rng.choice(EMIT_CAP, (1 << 16) + 64, replace=False)]))
        drop = np.setdiff1d(ids, must)[:ids.size - (1 << 16)]
        ids = np.setdiff1d(ids, drop)
        assert ids.size == 1 << 16 and np.isin(must, ids).all()
        ids = ids[rng.permutation(ids.size)]
        o = rng.permutation(ids.size - 1)
        s, d = ids[o], ids[o + 1]
        _EMIT["s"], _EMIT["d"] = s, d
        _EMIT["ref"] = _ref_of(s, d, EMIT_CAP)
        assert _EMIT["ref"].status == (True, 1 << 16, 1)
    return _EMIT["s"], _EMIT["d"], _EMIT["ref"]


def _emit(c, v, k, s, cap):
    """gs_bip_emit_pairs -> (return code, n_out); v, k, s: pointers (or None)."""
    got = U64()
    rc = _abi.lib().gs_bip_emit_pairs(c.handle, ctypes.c_void_p(v), ctypes.c_void_p(k), ctypes.c_void_p(s), int(cap),
                                      ctypes.byref(got))
    return rc, int(got.value)


@pytest.mark.parametrize("bits", [32, 64])
def test_emission_two_tiles_per_scan_thread(torch_cuda, bits):
    torch = torch_cuda
    assert (EMIT_CAP + 4095) // 4096 == 1026 and EMIT_CAP % 4096 == 1
    s, d, ref = _emit_case()
    c = Candidates(EMIT_CAP, id_bits=bits)
    rc, n = _emit(c, None, None, None, 0)                           # empty summary, null outputs
    assert (rc, n) == (_abi.GS_OK, 0)
    c.fold(s, d)
    _check(c, ref)
    hv, hk, hs = c.pairs()
    total = ref.n_vertices
    # straight into device buffers
    tdt = torch.int32 if bits == 32 else torch.int64
    dv, dk = torch.zeros(total, dtype=tdt, device="cuda"), torch.zeros(total, dtype=tdt, device="cuda")
    dsg = torch.zeros(total, dtype=torch.uint8, device="cuda")
    rc, n = _emit(c, dv.data_ptr(), dk.data_ptr(), dsg.data_ptr(), total)
    assert (rc, n) == (_abi.GS_OK, total)
    torch.cuda.synchronize()
    assert np.array_equal(dv.cpu().numpy().astype(np.int64), hv) and np.array_equal(dk.cpu().numpy().astype(np.int64), hk)
    assert np.array_equal(dsg.cpu().numpy().astype(bool), hs)
    # cap = total - 1 into buffers of total elements, pre-filled with a marker: device, then host
    dv.fill_(-7)
    dk.fill_(-7)
    dsg.fill_(0xEE)
    rc, n = _emit(c, dv.data_ptr(), dk.data_ptr(), dsg.data_ptr(), total - 1)
    assert (rc, n) == (_abi.GS_ERR_CAPACITY, total)
    torch.cuda.synchronize()
    gv, gk, gs = dv.cpu().numpy().astype(np.int64), dk.cpu().numpy().astype(np.int64), dsg.cpu().numpy()
    assert np.array_equal(gv[:-1], hv[:-1]) and np.array_equal(gk[:-1], hk[:-1]) and np.array_equal(gs[:-1].astype(bool), hs[:-1])
    assert (gv[-1], gk[-1], gs[-1]) == (-7, -7, 0xEE)
    ndt = np.uint32 if bits == 32 else np.int64
    nv, nk, ns = np.full(total, 77, dtype=ndt), np.full(total, 77, dtype=ndt), np.full(total, 0xEE, dtype=np.uint8)
    rc, n = _emit(c, nv.ctypes.data, nk.ctypes.data, ns.ctypes.data, total - 1)
    assert (rc, n) == (_abi.GS_ERR_CAPACITY, total)
    assert np.array_equal(nv[:-1].astype(np.int64), hv[:-1]) and np.array_equal(nk[:-1].astype(np.int64), hk[:-1])
    assert np.array_equal(ns[:-1].astype(bool), hs[:-1]) and (nv[-1], nk[-1], ns[-1]) == (77, 77, 0xEE)
    rc, n = _emit(c, None, None, None, 0)                           # non-empty summary, null outputs
    assert (rc, n) == (_abi.GS_ERR_CAPACITY, total)
    _check(c, ref)                                                  # the summary is as it was
    c.close()


# ---- 6. tiny capacities: the young split at cap / 4 == 0 and == 1 ----
def _tiny_edge_lists(cap):
    loops = [(v, v) for v in range(cap)]
    cross = [(a, b) for a in range(cap) for b in range(a + 1, cap) if (a ^ b) & 1]     # even - odd: bipartite
    every = [(a, b) for a in range(cap) for b in range(a + 1, cap)]                      # complete graph
    out = {"loops": loops, "cross": loops + cross, "cross_rev": [(b, a) for a, b in reversed(loops + cross)],
           "cross_first": cross + loops, "complete": loops + every, "complete_rev": [(b, a) for a, b in reversed(every)]}
    return {k: v for k, v in out.items() if v}


def _uf_string(edges):
    uf = ParityUnionFind()
    for a, b in edges:
        uf.union(a, b)
    return emission_string(*uf.emission())


@pytest.mark.parametrize("cap", [1, 2, 3, 4, 5, 7])
def test_tiny_capacities(cap):
    """All self-loops and all edges that fit (the bipartite even-odd ones, and all of them), in two
    orders, both id widths, two-array and pair folds, in one call and one edge per call (the first
    launches of a handle hold max(cap / 4, 1) = 1 edge)."""
    for bits in (32, 64):
        dt = np.uint32 if bits == 32 else np.int64
        c = Candidates(cap, id_bits=bits)
        for what, edges in _tiny_edge_lists(cap).items():
            want = _uf_string(edges)
            if what.startswith("complete") and cap >= 3:
                assert want == "(false,{})"
            e = np.array(edges, dtype=dt).reshape(-1, 2)
            for how in ("arrays", "pairs", "arrays_one_by_one", "pairs_one_by_one"):
                c.reset()
                if how == "arrays":
                    c.fold(np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1]))
                elif how == "pairs":
                    _fold_pairs(c, e.ctypes.data, len(e))
                else:
                    for i in range(len(e)):
                        if how == "arrays_one_by_one":
                            c.fold(e[i:i + 1, 0].copy(), e[i:i + 1, 1].copy())
                        else:
                            _fold_pairs(c, e[i:i + 1].ctypes.data, 1)
                c.close_window()
                assert c.toString() == want, (cap, bits, what, how)
        c.close()
    if cap == 3:
        t = Candidates(3)
        t.fold(np.array([0, 1, 2]), np.array([1, 2, 0]))
        assert t.toString() == "(false,{})" and t.getMap() == {}
        t.close()


# ---- 7. the host staging loop across its 2^22-edge chunk ----
@pytest.mark.parametrize("bits", [32, 64])
def test_host_staging_chunk_boundary(bits):
    s, d = bs.staging_stream()
    assert s.size == (1 << 22) + 5 and s.dtype == np.int64
    c = Candidates(bs.L_FULL, id_bits=bits)
    if bits == 32:
        c.fold(s.astype(np.uint32), d.astype(np.uint32))
    else:
        c.fold(s, d)
    assert c.status() == (True, bs.L_FULL, 1)
    v, k, sg = c.pairs()
    assert np.array_equal(v, np.arange(bs.L_FULL)) and not k.any() and np.array_equal(sg, bs.hypercube_sign(bs.L_FULL))
    assert c.checksum()[0] == bs.checksum(v, k, bs.hypercube_sign(bs.L_FULL))
    c.close()


# ---- 8. the stream bench.py --workload bip times ----
def test_bench_shaped_stream(torch_cuda):
    torch = torch_cuda
    from gsgpu import gen
    st = bs.stream("rmat_sides")
    refs = bs.reference_windows("rmat_sides")
    assert len(refs) == 16
    n = st.src.size
    s = torch.empty(n, dtype=torch.int32, device="cuda")
    d = torch.empty(n, dtype=torch.int32, device="cuda")
    gen.rmat(s, d, 0, st.info["scale"], bs.RMAT_SEED)
    s.mul_(2)
    d.mul_(2).add_(1)
    torch.cuda.synchronize()
    assert np.array_equal(s.cpu().numpy().astype(np.int64), st.src) and np.array_equal(d.cpu().numpy().astype(np.int64), st.dst)
    c = Candidates(st.cap, id_bits=32, stream=torch.cuda.current_stream())
    for w, ref in enumerate(refs):
        lo = w * st.W
        c.fold(s[lo:lo + st.W], d[lo:lo + st.W])
        c.close_window()
        assert c.checksum() == (ref.checksum, True, ref.n_vertices, ref.n_components), "window %d" % w
        assert c.status() == ref.status
    _check(c, refs[-1])
    v, k, sg = c.pairs()
    assert np.array_equal(sg, (v & 1) == (k & 1))
    c.close()


# ---- 9. checkpoint on deep state ----
@pytest.mark.parametrize("name,after", [("shuffled_path", 3), ("matching_loops", 3), ("odd_cycle_mid", 4)])
def test_checkpoint_on_deep_state(name, after):
    """snapshot() after `after` windows, restore into a new handle in shuffled entry order, then the
    rest of the stream: every later window equals the reference. odd_cycle_mid: the snapshot is
    failed and stays failed."""
    st = bs.stream(name)
    refs = bs.reference_windows(name)
    c = Candidates(st.cap)
    for w in range(after):
        c.fold(st.src[w * st.W:(w + 1) * st.W], st.dst[w * st.W:(w + 1) * st.W])
        c.close_window()
    ok, v, k, sg = c.snapshot()
    assert ok == refs[after - 1].ok and v.size == refs[after - 1].n_vertices
    assert ok == (name != "odd_cycle_mid")
    c.close()
    o = np.random.default_rng(302).permutation(v.size)
    c2 = Candidates(st.cap)
    c2.restore(ok, v[o], k[o], sg[o])
    _check(c2, refs[after - 1], "restored")
    for w in range(after, len(refs)):
        c2.fold(st.src[w * st.W:(w + 1) * st.W], st.dst[w * st.W:(w + 1) * st.W])
        c2.close_window()
        _check(c2, refs[w], "window %d" % w)
    c2.close()


# ---- 10. literal mode, small (one workgroup: it stays tiny) ----
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("name", ["asc_path", "shuffled_path", "odd_cycle", "matching_loops"])
def test_literal_mode_small(name, P):
    st = bs.stream(name, bs.L_TINY)
    assert (st.cap, st.W) == (259, 32)
    want = literal_run(st.src, st.dst, st.W, partitions=P)
    got = [c.toString() for c in SimpleEdgeStream(st.src, st.dst).aggregate(
        BipartitenessCheck(1000, window_edges=st.W, mode="literal", parallelism=P, vertex_capacity=st.cap,
                           entry_capacity=1 << 16))]
    assert got == want
