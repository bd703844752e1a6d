"""GPU: neighbourhood slices (gs_slice_*, gsgpu.SnapshotStream) against oracle (a) of
tests/slices_oracle.py, exactly: the reference's nine known answers, random and structured streams
(tests/slice_streams.py), value edge cases, lifecycle, errors and the multi-window call. Unless a
test says otherwise it covers six ops x three directions x id_bits 32 and 64; every slice is also
read back as CSR and through its statistics."""
import json
import os

import numpy as np
import pytest

import slice_streams as S
import slices_oracle as O
from gsgpu import GsError, SimpleEdgeStream, SnapshotStream, _abi
from test_slices_oracle import kat_lines

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "slice_kat.json")))
EDGES = np.array(KAT["edges"], dtype=np.int64)
SRC, DST, VAL = EDGES[:, 0], EDGES[:, 1], EDGES[:, 2]


def check_slice(ss, src, dst, val, ops=O.OPS):
    """The slice `ss` holds (built from these edges) equals oracle (a): every op, CSR, statistics."""
    d = ss.direction
    rows = O.reference_rows(src, dst, val, d)
    for op in ops:
        v, x = ss.reduce_on_edges(op)
        assert v.dtype == (np.uint32 if ss.id_bits == 32 else np.int64) and x.dtype == np.int64
        assert list(zip(v.tolist(), x.tolist())) == O.reference_reduce(rows, op), (d, ss.id_bits, op)
        assert ss.stats(op) == O.reference_stats(rows, op), (d, ss.id_bits, op)
    v, o, nb, x = ss.rows()
    wv, wo, wn, wx = O.reference_csr(rows)
    assert (v.tolist(), o.tolist(), nb.tolist()) == (wv, wo, wn), (d, ss.id_bits)
    assert (x is None and wx is None) or x.tolist() == wx, (d, ss.id_bits)


def check_stream(src, dst, val, cap, directions=O.DIRECTIONS, bits=(32, 64), ops=O.OPS):
    for id_bits in bits:
        for d in directions:
            with SnapshotStream(cap, d, id_bits=id_bits) as ss:
                check_slice(ss.window(src, dst, val), src, dst, val, ops)


# ---- the reference's known answers ----
@pytest.mark.parametrize("id_bits", [32, 64])
@pytest.mark.parametrize("case", KAT["cases"], ids=[c["name"] for c in KAT["cases"]])
def test_known_answers(case, id_bits):
    with SnapshotStream(6, case["direction"], id_bits=id_bits) as ss:
        ss.window(SRC, DST, VAL)
        got = kat_lines(case, lambda d, op: list(zip(*[a.tolist() for a in ss.reduce_on_edges(op)])), lambda d: ss.rows())
        assert got == case["expected"]                           # (emitted ordered by vertex)
        if case["operator"] == "apply":
            label = lambda v, nb, x: "%d,%s" % (v, "big" if int(x.sum()) > KAT["apply_threshold"] else "small")
            assert ss.apply_on_neighbors(label) == case["expected"]
        if case["operator"] == "fold":
            got = ss.fold_neighbors(0, lambda acc, v, nb, x: acc + x)
            assert ["%d,%d" % r for r in got] == case["expected"]


def test_slice_of_a_simple_edge_stream():
    st = SimpleEdgeStream(np.tile(SRC, 2), np.tile(DST, 2), values=np.concatenate([VAL, 2 * VAL]))
    got = [list(zip(*[a.tolist() for a in ss.reduce_on_edges("sum")])) for ss in st.slice(window_edges=7, direction="all")]
    want = [(1, 76), (2, 35), (3, 105), (4, 79), (5, 131)]
    assert got == [want, [(v, 2 * x) for v, x in want]]
    timed = SimpleEdgeStream(SRC, DST, timestamps=[0, 1, 2, 1000, 1001, 1002, 2500], values=VAL)
    got = [ss.reduce_on_edges("count")[1].tolist() for ss in timed.slice(1000)]
    assert got == [[2, 1], [2, 1], [1]]


# ---- random streams ----
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 4097])
def test_random_streams(n):
    check_stream(*S.rmat(12, n, 100 + n))
    check_stream(*S.uniform(5, n, 200 + n))
    check_stream(*S.uniform(4097, n, 300 + n))
    check_stream(*S.uniform((1 << 21) + 1, n, 400 + n))                 # ids past 16 bits and past 2^21


# ---- row shapes ----
def test_row_shapes():
    s, d, x, cap = S.row_shapes()
    assert np.any(np.diff(s) < 0)
    check_stream(s, d, x, cap)
    check_stream(*S.tile_seams())


@pytest.mark.parametrize("fillers", [range(1, 17), range(17, 33), range(33, 49), range(49, 64)], ids=lambda r: "%d-%d" % (r[0], r[-1]))
def test_row_shapes_at_every_lane_position(fillers):
    """The row lengths shifted by 1..63 filler entries ("out", 64-bit ids, every op)."""
    with SnapshotStream(64, "out") as ss:
        for f in fillers:
            s, d, x, _ = S.row_shapes(f)
            check_slice(ss.window(s, d, x), s, d, x)


@pytest.mark.parametrize("n", [1, 64, 65, 2048, 2049, 5000])
def test_distinct_vertices(n):
    check_stream(*S.distinct(n), directions=("out",))


# ---- hubs ----
@pytest.mark.parametrize("family", ["hub", "hub_and_singles", "two_hubs"])
def test_hub_rows(family):
    """One row over many workgroups of the reduce kernel ("out", 64-bit ids, every op)."""
    s, d, x, cap = getattr(S, family)()
    assert s.size >= S.HUB_EDGES >= 8 * S.TILE
    check_stream(s, d, x, cap, directions=("out",), bits=(64,))


def test_hub_rows_under_all():
    s, d, x, cap = S.hub(20000)
    check_stream(s, d, x, cap, directions=("all", "in"), bits=(32,))


# ---- values ----
@pytest.mark.parametrize("name", sorted(S.value_cases()))
def test_value_cases(name):
    check_stream(*S.value_cases()[name])


def test_long_rows_of_extreme_values():
    """Wrapping sums and signed minima / maxima across waves and workgroups."""
    g = np.random.default_rng(5)
    n = 3 * S.TILE + 17
    src = g.integers(0, 2, size=n, dtype=np.int64)
    dst = g.integers(0, 2, size=n, dtype=np.int64)
    for x in (np.full(n, S.I64_MAX), np.full(n, S.I64_MIN), g.choice(np.array([S.I64_MIN, S.I64_MAX, -1, 0, 1]), size=n),
              -1 - g.integers(0, 1000, size=n, dtype=np.int64)):
        check_stream(src, dst, x.astype(np.int64), 2, bits=(64,))


# ---- slices without values ----
@pytest.mark.parametrize("direction", O.DIRECTIONS)
def test_no_values(direction):
    s, d, _, cap = S.rmat(12, 1000, 77)
    with SnapshotStream(cap, direction) as ss:
        ss.window(s, d)
        check_slice(ss, s, d, None, ops=("count",))
        for op in ("sum", "min", "max", "first", "last"):
            with pytest.raises(GsError) as ei:
                ss.reduce_on_edges(op)
            assert ei.value.code == _abi.GS_ERR_INVALID
            with pytest.raises(GsError) as ei:
                ss.reduce_windows(s, d, None, 100, op)
            assert ei.value.code == _abi.GS_ERR_INVALID
        recs, _ = ss.reduce_windows(s, d, None, 400, "count")
        for k, (v, c) in enumerate(recs):
            rows = O.reference_rows(s[400 * k:400 * k + 400], d[400 * k:400 * k + 400], None, direction)
            assert list(zip(v.tolist(), c.tolist())) == O.reference_reduce(rows, "count")


# ---- lifecycle ----
@pytest.mark.parametrize("direction", O.DIRECTIONS)
def test_empty_window(direction):
    e = np.zeros(0, dtype=np.int64)
    with SnapshotStream(10, direction) as ss:
        ss.window(e, e, e)
        for op in O.OPS:
            v, x = ss.reduce_on_edges(op)
            assert v.size == 0 and x.size == 0
            assert ss.stats(op) == {"n_vertices": 0, "n_entries": 0, "max_row": 0, "checksum": 0}
        v, o, nb, x = ss.rows()
        assert (v.size, o.tolist(), nb.size, x.size) == (0, [0], 0, 0)
        recs, st = ss.reduce_windows(e, e, e, 5, "sum")
        assert recs == [] and st.size == 0
        ss.window(SRC, DST, VAL)                                  # and a window after the empty one
        check_slice(ss, SRC, DST, VAL)
        ss.window(e, e, e)
        assert ss.reduce_on_edges("sum")[0].size == 0


@pytest.mark.parametrize("direction", O.DIRECTIONS)
def test_handle_reuse_leaves_nothing_stale(direction):
    """Windows of growing and shrinking size over disjoint vertex sets on one handle."""
    cap = 40000
    with SnapshotStream(cap, direction, id_bits=32) as ss:
        for k, n in enumerate([10, 5000, 70, 20000, 3, 4097, 1]):
            s, d, x, _ = S.uniform(5000, n, 900 + k)
            s, d = s + 5000 * k, d + 5000 * k
            check_slice(ss.window(s, d, x), s, d, x)


@pytest.mark.parametrize("id_bits", [32, 64])
def test_device_inputs_and_outputs(id_bits):
    import torch
    s, d, x, cap = S.rmat(12, 5000, 55)
    dt = torch.int32 if id_bits == 32 else torch.int64
    ds, dd = torch.from_numpy(s).to("cuda").to(dt), torch.from_numpy(d).to("cuda").to(dt)
    dx = torch.from_numpy(x).to("cuda")
    for direction in O.DIRECTIONS:
        rows = O.reference_rows(s, d, x, direction)
        ne = 2 * s.size if direction == "all" else s.size
        with SnapshotStream(cap, direction, id_bits=id_bits) as ss:
            check_slice(ss.window(ds, dd, dx), s, d, x)
            ov = torch.full((ne,), 7, dtype=dt, device="cuda")
            ox = torch.full((ne,), -7, dtype=torch.int64, device="cuda")
            for op in O.OPS:
                n = ss.reduce_on_edges(op, out=(ov, ox))
                assert list(zip(ov[:n].tolist(), ox[:n].tolist())) == O.reference_reduce(rows, op)
                assert n == len(rows) and (n == ne or (int(ov[n]) == 7 and int(ox[n]) == -7))
            oo = torch.zeros(len(rows) + 1, dtype=torch.int64, device="cuda")
            on = torch.zeros(ne, dtype=dt, device="cuda")
            nv, got_ne = ss.rows(out=(ov, oo, on, ox))
            wv, wo, wn, wx = O.reference_csr(rows)
            assert (nv, got_ne) == (len(wv), ne)
            assert (ov[:nv].tolist(), oo.tolist(), on.tolist(), ox.tolist()) == (wv, wo, wn, wx)
            offs, st = ss.reduce_windows(ds, dd, dx, 1000, "max", out=(ov, ox))
            for k in range(5):
                w = slice(1000 * k, 1000 * k + 1000)
                want = O.reference_reduce(O.reference_rows(s[w], d[w], x[w], direction), "max")
                a, b = int(offs[k]), int(offs[k + 1])
                assert list(zip(ov[a:b].tolist(), ox[a:b].tolist())) == want


def test_own_stream_waits_for_torch():
    """The handle runs on its own stream; its inputs are still being produced on torch's."""
    import torch
    s, d, x, cap = S.rmat(12, 1 << 16, 66)
    base = [torch.from_numpy(a).to("cuda") for a in (s, d, x)]
    with SnapshotStream(cap, "all") as ss:
        filler = torch.rand(1 << 24, device="cuda")
        for _ in range(4):
            filler = torch.sort(filler).values.flip(0)            # work queued in front of the inputs
        ds, dd, dx = [(t + 1) - 1 for t in base]                  # produced behind it, in torch's stream order
        ss.window(ds, dd, dx)
        check_slice(ss, s, d, x, ops=("sum", "last"))
    with SnapshotStream(cap, "all", stream=torch.cuda.current_stream()) as ss:
        check_slice(ss.window(ds, dd, dx), s, d, x, ops=("min",))


# ---- errors ----
@pytest.mark.parametrize("id_bits", [32, 64])
@pytest.mark.parametrize("direction", O.DIRECTIONS)
def test_out_of_range_ids(direction, id_bits):
    s, d, x, cap = S.uniform(100, 500, 88)
    with SnapshotStream(cap, direction, id_bits=id_bits) as ss:
        bad = [(cap, 3)] + ([(-1, 7)] if id_bits == 64 else [])
        for v, at in bad:
            for side in (0, 1):
                t = [s.copy(), d.copy()]
                t[side][at] = v
                with pytest.raises(GsError) as ei:
                    ss.window(t[0], t[1], x)
                assert ei.value.code == _abi.GS_ERR_RANGE
                assert ss.reduce_on_edges("count")[0].size == 0   # the handle holds an empty slice
                check_slice(ss.window(s, d, x), s, d, x)          # and the next window is right
        t = np.concatenate([s, s])
        t[700] = cap
        with pytest.raises(GsError) as ei:
            ss.reduce_windows(t, np.concatenate([d, d]), np.concatenate([x, x]), 250, "sum")
        assert ei.value.code == _abi.GS_ERR_RANGE
        check_slice(ss.window(s, d, x), s, d, x)


def test_unknown_op_and_direction():
    import ctypes
    h = ctypes.c_void_p()
    assert _abi.lib().gs_slice_create(ctypes.byref(h), 10, 64, 0, 3) == _abi.GS_ERR_INVALID
    with pytest.raises(ValueError):
        SnapshotStream(10, "both")
    with SnapshotStream(10) as ss:
        ss.window(SRC, DST, VAL)
        for op in (-1, 6):
            with pytest.raises(GsError) as ei:
                ss.reduce_on_edges(op)
            assert ei.value.code == _abi.GS_ERR_INVALID
            with pytest.raises(GsError) as ei:
                ss.stats(op)
            assert ei.value.code == _abi.GS_ERR_INVALID
        with pytest.raises(ValueError):
            ss.reduce_on_edges("mean")


@pytest.mark.parametrize("device_out", [False, True])
def test_capacity_one_short_writes_nothing(device_out):
    import ctypes
    import torch
    s, d, x, cap = S.rmat(12, 3000, 99)
    with SnapshotStream(cap, "all") as ss:
        ss.window(s, d, x)
        need = len(O.reference_rows(s, d, x, "all"))
        if device_out:
            v = torch.full((need,), -5, dtype=torch.int64, device="cuda")
            r = torch.full((need,), -6, dtype=torch.int64, device="cuda")
            pv, pr = ctypes.c_void_p(v.data_ptr()), ctypes.c_void_p(r.data_ptr())
        else:
            v, r = np.full(need, -5, dtype=np.int64), np.full(need, -6, dtype=np.int64)
            pv, pr = v.ctypes.data_as(ctypes.c_void_p), r.ctypes.data_as(ctypes.c_void_p)
        n = ctypes.c_uint64()
        L = _abi.lib()
        assert L.gs_slice_reduce(ss.handle, _abi.GS_SLICE_SUM, pv, pr, need - 1, ctypes.byref(n)) == _abi.GS_ERR_CAPACITY
        assert n.value == need
        assert set(v.tolist()) == {-5} and set(r.tolist()) == {-6}              # the sentinel fill is untouched
        nv, ne = ctypes.c_uint64(), ctypes.c_uint64()
        o = np.full(need + 1, 9, dtype=np.uint64)
        nb = np.full(2 * s.size, -4, dtype=np.int64)
        xs = np.full(2 * s.size, -3, dtype=np.int64)
        args = (o.ctypes.data_as(ctypes.c_void_p), nb.ctypes.data_as(ctypes.c_void_p), xs.ctypes.data_as(ctypes.c_void_p))
        assert L.gs_slice_rows(ss.handle, pv, *args, need - 1, 2 * s.size, ctypes.byref(nv), ctypes.byref(ne)) == _abi.GS_ERR_CAPACITY
        assert L.gs_slice_rows(ss.handle, pv, *args, need, 2 * s.size - 1, ctypes.byref(nv), ctypes.byref(ne)) == _abi.GS_ERR_CAPACITY
        assert (nv.value, ne.value) == (need, 2 * s.size)
        assert set(v.tolist()) == {-5} and set(o.tolist()) == {9} and set(nb.tolist()) == {-4} and set(xs.tolist()) == {-3}
        assert L.gs_slice_reduce(ss.handle, _abi.GS_SLICE_SUM, pv, pr, need, ctypes.byref(n)) == _abi.GS_OK
        assert list(zip(v.tolist(), r.tolist())) == O.reference_reduce(O.reference_rows(s, d, x, "all"), "sum")


# ---- every window in one call ----
@pytest.mark.parametrize("id_bits", [32, 64])
@pytest.mark.parametrize("direction", O.DIRECTIONS)
def test_reduce_windows_equals_per_window_calls(direction, id_bits):
    s, d, x, cap, W = S.multi_window()
    nw = -(-s.size // W)
    assert nw == 11 and s.size % W
    with SnapshotStream(cap, direction, id_bits=id_bits) as ss, SnapshotStream(cap, direction, id_bits=id_bits) as one:
        for op in O.OPS:
            recs, st = ss.reduce_windows(s, d, x, W, op)
            assert len(recs) == nw and st.size == nw
            for k in range(nw):
                w = slice(W * k, min(W * k + W, s.size))
                rows = O.reference_rows(s[w], d[w], x[w], direction)
                assert list(zip(recs[k][0].tolist(), recs[k][1].tolist())) == O.reference_reduce(rows, op), (op, k)
                one.window(s[w], d[w], x[w])
                v1, x1 = one.reduce_on_edges(op)
                assert (v1.tolist(), x1.tolist()) == (recs[k][0].tolist(), recs[k][1].tolist())
                assert {f: int(st[k][f]) for f in st.dtype.names} == one.stats(op) == O.reference_stats(rows, op)
        w = slice(W * (nw - 1), s.size)                            # the handle holds the call's last window
        check_slice(ss, s[w], d[w], x[w])


def test_reduce_windows_capacities():
    import ctypes
    s, d, x, cap, W = S.multi_window()
    nw = -(-s.size // W)
    L = _abi.lib()
    with SnapshotStream(cap, "out") as ss:
        recs, _ = ss.reduce_windows(s, d, x, W, "sum")
        total = sum(len(v) for v, _ in recs)
        v, r = np.full(total, -5, dtype=np.int64), np.full(total, -6, dtype=np.int64)
        offs, st = np.full(nw + 1, 9, dtype=np.uint64), np.zeros(4 * nw, dtype=np.uint64)
        got = ctypes.c_uint64()
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = L.gs_slice_reduce_windows(ss.handle, p(s), p(d), p(x), s.size, W, _abi.GS_SLICE_SUM, p(v), p(r), total, p(offs), p(st),
                                       nw - 1, ctypes.byref(got))
        assert rc == _abi.GS_ERR_CAPACITY and got.value == nw                  # one window short: nothing is run
        assert set(v.tolist()) == {-5} and set(r.tolist()) == {-6} and set(offs.tolist()) == {9}
        rc = L.gs_slice_reduce_windows(ss.handle, p(s), p(d), p(x), s.size, W, _abi.GS_SLICE_SUM, p(v), p(r), total - 1, p(offs), p(st),
                                       nw, ctypes.byref(got))
        assert rc == _abi.GS_ERR_CAPACITY                                      # the records outgrow cap
        rc = L.gs_slice_reduce_windows(ss.handle, p(s), p(d), p(x), s.size, W, _abi.GS_SLICE_SUM, p(v), p(r), total, p(offs), p(st),
                                       nw, ctypes.byref(got))
        assert rc == _abi.GS_OK and int(offs[nw]) == total
        assert v.tolist() == np.concatenate([a for a, _ in recs]).tolist()
        assert r.tolist() == np.concatenate([b for _, b in recs]).tolist()
