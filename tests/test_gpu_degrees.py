"""GPU parity of the streaming degrees (gs_deg_*): the reference's known answers
(DegreeDistributionITCase, TestGetDegrees), random event streams with deletions below zero equal to
the CPU oracle after every window, contention on one vertex, the dense / sparse cut of the
distribution, failures that leave the summary unchanged, and the checkpoint. Every case runs the
default flags (sort everything, as GS_DEG_SORT_ALL) and the counting path (GS_DEG_COUNT). Integer path: every comparison is exact."""
import collections
import ctypes
import functools
import json
import os

import numpy as np
import pytest

from gsgpu import DegreeDistribution, DegreeSummary, GsError, SimpleEdgeStream
from gsgpu import _abi
from degrees_oracle import ALL, IN, OUT, WindowOracle, random_events, reference_distribution

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KAT = json.load(open(os.path.join(GOLD, "degrees_kat.json")))
PATHS = [None, "count"]     # default flags (sort everything, the path of GS_DEG_SORT_ALL) and the counting path


def multiset(lines):
    return collections.Counter(tuple(int(y) for y in x) for x in lines)


def check(ds, rec, deltas=True):
    """The handle's summary equals the oracle's record of the same window."""
    v, d = ds.degrees()
    assert (v.tolist(), d.tolist()) == rec["degrees"]
    k, c = ds.distribution()
    assert (k.tolist(), c.tolist()) == rec["distribution"]
    assert ds.stats() == rec["stats"]
    if deltas:
        v, d = ds.degrees_delta()
        assert (v.tolist(), d.tolist()) == rec["degrees_delta"]
        k, c = ds.distribution_delta()
        assert (k.tolist(), c.tolist()) == rec["distribution_delta"]


# ---- 1. known answers ----
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", ["degree_distribution", "degree_distribution_zero"])
def test_degree_distribution_known_answers(name, path):
    """One-event windows. A window's distribution delta is the reference's last record of every key
    whose count the event changed; its records for a key that ends the event where it began (count[1]
    in "2 3 +": 2 -> 1 -> 2) are by definition not emitted. The emitted lines and those make up the
    reference's expected lines, line for line."""
    k = KAT[name]
    e = np.asarray(k["events"], dtype=np.int64)
    stream = SimpleEdgeStream(e[:, 0], e[:, 1], events=e[:, 2])
    got = list(DegreeDistribution(window_edges=1, path=path, dense_degrees=4).run(stream))
    _, per, _ = reference_distribution(k["events"])
    before = {}
    unreproduced = []
    for i, records in enumerate(per):
        last, after = {}, dict(before)
        for d, c in records:
            last[d] = c
            after[d] = c
        want = sorted((d, c) for d, c in last.items() if before.get(d, 0) != c)
        assert got[i] == want, i
        counted = collections.Counter(records)
        counted.subtract(want)
        unreproduced += list(counted.elements())
        before = after
    assert multiset([x for w in got for x in w]) + multiset(unreproduced) == multiset(k["expected"])


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name,method", [("degrees", "getDegrees"), ("in_degrees", "getInDegrees"),
                                         ("out_degrees", "getOutDegrees")])
def test_get_degrees_known_answers(name, method, path):
    k = KAT["get_degrees"]
    e = np.asarray(k["edges"], dtype=np.int64)
    stream = SimpleEdgeStream(e[:, 0], e[:, 1])
    got = [x for w in getattr(stream, method)(1, path=path) for x in w]
    assert multiset(got) == multiset(k[name])
    got32 = [x for w in getattr(stream, method)(1, path=path, id_bits=32) for x in w]
    assert multiset(got32) == multiset(k[name])


# ---- 2. random multigraph event streams, self-loops kept ----
STREAMS = [(3, 40, 1), (8, 200, 7), (40, 610, 150), (1000, 20000, 257), (1 << 14, 1 << 18, 1 << 16)]
P_ADD = [1.0, 0.9, 0.5]


@functools.lru_cache(maxsize=None)
def _stream_and_oracle(nv, n, W, p, dirs=ALL):
    src, dst, add = random_events(nv, n, p, seed=31 * nv + n + int(10 * p))
    orc = WindowOracle(nv, dirs)
    recs = tuple(orc.fold(src[lo:lo + W], dst[lo:lo + W], add[lo:lo + W]) for lo in range(0, n, W))
    for a in (src, dst, add):
        a.setflags(write=False)
    return src, dst, add, recs, orc


def _cases():
    out = []
    for nv, n, W in STREAMS:
        for p in P_ADD:
            for path in PATHS:
                for id_bits in ((32, 64) if n <= 20000 else (32,)):
                    out.append((nv, n, W, p, path, id_bits))
    return out


@pytest.mark.parametrize("nv,n,W,p,path,id_bits", _cases())
def test_random_streams_equal_the_oracle(nv, n, W, p, path, id_bits):
    src, dst, add, recs, orc = _stream_and_oracle(nv, n, W, p)
    assert np.any(src == dst) and len(recs) == -(-n // W)
    assert orc.plain_sum_broken == 0
    if p == 0.5:
        assert orc.clamped > 0                      # a stream that never clamps shows nothing
    if p == 1.0:
        assert orc.risk_windows == 0 and orc.clamped == 0
    dense = 0 if nv == 1 << 14 else 4               # the default cut on the largest stream
    with DegreeSummary(nv, id_bits=id_bits, path=path, dense_degrees=dense) as ds:
        for w, lo in enumerate(range(0, n, W)):
            ds.fold_window(src[lo:lo + W], dst[lo:lo + W], None if p == 1.0 else add[lo:lo + W])
            check(ds, recs[w])
        ids = np.arange(min(nv, 64))
        want = dict(zip(*recs[-1]["degrees"]))
        assert ds.find(ids).tolist() == [want.get(int(i), 0) for i in ids]
    if n % W:
        assert n - (len(recs) - 1) * W < W          # the last window is short


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("direction,dirs", [("in", IN), ("out", OUT)])
def test_directions(direction, dirs, path):
    nv, n, W, p = 40, 610, 150, 0.5
    src, dst, add, recs, orc = _stream_and_oracle(nv, n, W, p, dirs)
    with DegreeSummary(nv, direction=direction, path=path, dense_degrees=4) as ds:
        for w, lo in enumerate(range(0, n, W)):
            ds.fold_window(src[lo:lo + W], dst[lo:lo + W], add[lo:lo + W])
            check(ds, recs[w])


# ---- 3. contention and combining ----
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_every_event_on_one_vertex(n, path):
    hub = 5
    with DegreeSummary(8192, id_bits=32, path=path, dense_degrees=4) as ds:
        orc = WindowOracle(8192)
        s = np.full(n, hub, dtype=np.int64)
        rec = orc.fold(s, s)                                   # self-loops: 2 n
        ds.fold_window(s, s)
        check(ds, rec)
        assert rec["degrees"] == ([hub], [2 * n])
        leaves = 6 + np.arange(n, dtype=np.int64)              # a star
        rec = orc.fold(s, leaves)
        ds.fold_window(s, leaves)
        check(ds, rec)
        assert ds.find([hub]).tolist() == [3 * n]
        rec = orc.fold(leaves, s, np.zeros(n, dtype=bool))     # and away again
        ds.fold_window(leaves, s, np.zeros(n, dtype=bool))
        check(ds, rec)
        assert rec["degrees"] == ([hub], [2 * n])


@pytest.mark.parametrize("path", PATHS)
def test_two_hubs_alternating_inside_a_wave(path):
    n = 640
    s = np.where(np.arange(n) % 2 == 0, 3, 9).astype(np.int64)
    d = np.where(np.arange(n) % 3 == 0, 9, 3).astype(np.int64)
    add = (np.arange(n) % 5 != 0)
    with DegreeSummary(16, path=path, dense_degrees=4) as ds:
        orc = WindowOracle(16)
        for lo in range(0, n, 128):
            rec = orc.fold(s[lo:lo + 128], d[lo:lo + 128], add[lo:lo + 128])
            ds.fold_window(s[lo:lo + 128], d[lo:lo + 128], add[lo:lo + 128])
            check(ds, rec)


@pytest.mark.parametrize("path", PATHS)
def test_long_run_with_one_clamp(path):
    """3,000 additions at one vertex, then 3,001 deletions in the next window: a long exact-path
    run whose last step clamps."""
    hub, n = 7, 3000
    leaves = 100 + np.arange(n + 1, dtype=np.int64)
    s = np.full(n + 1, hub, dtype=np.int64)
    orc = WindowOracle(8192, OUT)
    with DegreeSummary(8192, direction="out", path=path, dense_degrees=4) as ds:
        rec = orc.fold(s[:n], leaves[:n])
        ds.fold_window(s[:n], leaves[:n])
        check(ds, rec)
        assert rec["degrees"] == ([hub], [n])
        rec = orc.fold(s, leaves, np.zeros(n + 1, dtype=bool))
        ds.fold_window(s, leaves, np.zeros(n + 1, dtype=bool))
        check(ds, rec)
        assert rec["degrees"] == ([], []) and orc.clamped == 1
        # deletions first, then additions: the clamp is at the front of the run
        ev = np.concatenate([np.zeros(5, dtype=bool), np.ones(n, dtype=bool)])
        ss = np.full(n + 5, hub, dtype=np.int64)
        ll = 100 + np.arange(n + 5, dtype=np.int64)
        rec = orc.fold(ss, ll, ev)
        ds.fold_window(ss, ll, ev)
        check(ds, rec)
        assert rec["degrees"] == ([hub], [n])


# ---- 4. the dense / sparse cut of the distribution ----
@pytest.mark.parametrize("path", PATHS)
def test_distribution_cut(path):
    nv = 256
    with DegreeSummary(nv, path=path, dense_degrees=4) as ds:
        orc = WindowOracle(nv)

        def step(s, d, a=None):
            rec = orc.fold(s, d, a)
            ds.fold_window(np.asarray(s), np.asarray(d), None if a is None else np.asarray(a))
            check(ds, rec)
            return rec

        step([1, 1, 1], [2, 3, 4])                               # degree 3
        assert step([1], [5])["distribution_delta"] == ([1, 3, 4], [4, 0, 1])   # 3 -> 4: into the table
        assert step([1], [6])["distribution_delta"] == ([1, 4, 5], [5, 0, 1])   # 4 -> 5
        step([1, 1], [6, 5], [False, False])                     # 5 -> 3: back into the dense array
        assert orc.deg[1] == 3
        hub = 200
        leaves = np.arange(10, 110)
        rec = step(np.full(100, hub), leaves)                    # a hub of degree 100 appears
        assert 100 in rec["distribution"][0]
        rec = step(np.full(100, hub), leaves, np.zeros(100, dtype=bool))         # and leaves
        assert 100 not in rec["distribution"][0] and rec["distribution_delta"][0][-1] == 100
        assert rec["stats"]["max_degree"] == 3


@pytest.mark.parametrize("path", PATHS)
def test_many_sparse_keys_come_and_go(path):
    """One vertex climbs through 700 degrees in one-event windows: with dense_degrees = 4 every one
    of them is a key of the 256-slot table for one window, so the table is rebuilt on the way."""
    with DegreeSummary(2, direction="out", path=path, dense_degrees=4) as ds:
        orc = WindowOracle(2, OUT)
        for i in range(700):
            rec = orc.fold([0], [1])
            ds.fold_window(np.array([0]), np.array([1]))
            if i % 50 == 49 or i > 690:
                check(ds, rec)
        assert ds.stats()["max_degree"] == 700 and ds.stats()["n_degrees"] == 1


# ---- 5. a batch of windows in one call ----
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("p", [1.0, 0.5])
def test_fold_windows_equals_window_by_window(p, path):
    nv, n, W = 1000, 20000, 257
    src, dst, add, recs, _ = _stream_and_oracle(nv, n, W, p)
    ev = None if p == 1.0 else add
    with DegreeSummary(nv, id_bits=32, path=path, dense_degrees=4) as ds:
        for again in range(2):
            stats = ds.fold_windows(src, dst, W, ev)
            assert [{k: int(s[k]) for k in s.dtype.names} for s in stats] == [r["stats"] for r in recs]
            check(ds, recs[-1])
            ds.reset()
            assert ds.stats() == {"n_vertices": 0, "n_degrees": 0, "max_degree": 0, "checksum": 0}
            assert ds.degrees()[0].size == 0 and ds.distribution_delta()[0].size == 0
        # cap too small: nothing folded, nothing written
        nw = ctypes.c_uint64()
        mark = np.full((len(recs), 4), 0xDEADBEEF, dtype=np.uint64)
        s32, d32 = src.astype(np.uint32), dst.astype(np.uint32)
        rc = _abi.lib().gs_deg_fold_windows(ds.handle, s32.ctypes.data_as(ctypes.c_void_p), d32.ctypes.data_as(ctypes.c_void_p),
                                            None, n, W, mark.ctypes.data_as(ctypes.c_void_p), len(recs) - 1, ctypes.byref(nw))
        assert rc == _abi.GS_ERR_CAPACITY and nw.value == len(recs) and np.all(mark == 0xDEADBEEF)
        assert ds.stats()["n_vertices"] == 0
        assert ds.fold_windows(np.empty(0, dtype=np.int64), np.empty(0, dtype=np.int64), 10).size == 0
        with pytest.raises(ValueError):
            ds.fold_windows(src, dst, 0)


# ---- 6. failures leave the summary unchanged ----
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("id_bits", [32, 64])
def test_range_error_leaves_the_summary_unchanged(id_bits, path):
    nv, n, W, p = 40, 610, 150, 0.5
    src, dst, add, recs, _ = _stream_and_oracle(nv, n, W, p)
    with DegreeSummary(nv, id_bits=id_bits, path=path, dense_degrees=4) as ds:
        ds.fold_window(src[:W], dst[:W], add[:W])
        check(ds, recs[0])
        bad = src[W:2 * W].copy()
        bad[70] = nv                                             # an id equal to the capacity, mid-window
        with pytest.raises(GsError) as ei:
            ds.fold_window(bad, dst[W:2 * W], add[W:2 * W])
        assert ei.value.code == _abi.GS_ERR_RANGE
        check(ds, recs[0], deltas=False)
        ds.fold_window(src[W:2 * W], dst[W:2 * W], add[W:2 * W])
        check(ds, recs[1])
        if id_bits == 64:
            neg = src[2 * W:3 * W].copy()
            neg[0] = -1
            with pytest.raises(GsError) as ei:
                ds.fold_window(neg, dst[2 * W:3 * W], add[2 * W:3 * W])
            assert ei.value.code == _abi.GS_ERR_RANGE
            check(ds, recs[1], deltas=False)


@pytest.mark.parametrize("path", PATHS)
def test_restore_rejects_bad_snapshots(path):
    nv, n, W, p = 40, 610, 150, 0.9
    src, dst, add, recs, _ = _stream_and_oracle(nv, n, W, p)
    with DegreeSummary(nv, path=path, dense_degrees=4) as ds:
        ds.fold_window(src[:W], dst[:W], add[:W])
        for vs, degs, code in (([1, 2, 1], [1, 1, 1], _abi.GS_ERR_INVALID), ([1, 2], [1, 0], _abi.GS_ERR_INVALID),
                               ([1, nv], [1, 1], _abi.GS_ERR_RANGE)):
            with pytest.raises(GsError) as ei:
                ds.restore(vs, degs)
            assert ei.value.code == code
            check(ds, recs[0], deltas=False)
        ds.fold_window(src[W:2 * W], dst[W:2 * W], add[W:2 * W])
        check(ds, recs[1])


@pytest.mark.parametrize("path", PATHS)
def test_degrees_are_32_bits_wide(path):
    with DegreeSummary(8, path=path, dense_degrees=4) as ds:
        ds.restore([3], [2 ** 32 - 2])
        assert ds.stats()["max_degree"] == 2 ** 32 - 2 and ds.find([3]).tolist() == [2 ** 32 - 2]
        with pytest.raises(GsError) as ei:
            ds.fold_window(np.array([3]), np.array([4]))
        assert ei.value.code == _abi.GS_ERR_CAPACITY
        assert ds.degrees()[1].tolist() == [2 ** 32 - 2]
        assert ds.distribution()[0].tolist() == [2 ** 32 - 2]


# ---- 7. the checkpoint ----
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("id_bits", [32, 64])
def test_snapshot_restore_continue(id_bits, path):
    nv, n, W, p = 1000, 20000, 257, 0.5
    src, dst, add, recs, _ = _stream_and_oracle(nv, n, W, p)
    cut = 30
    with DegreeSummary(nv, id_bits=id_bits, path=path, dense_degrees=4) as a:
        a.fold_windows(src[:cut * W], dst[:cut * W], W, add[:cut * W])
        snap = a.snapshot()
    with DegreeSummary(nv, id_bits=id_bits, path=path, dense_degrees=4) as b:
        order = np.random.default_rng(1).permutation(snap[0].size)
        b.restore(snap[0][order], snap[1][order])
        check(b, recs[cut - 1], deltas=False)
        assert b.degrees_delta()[0].size == 0 and b.distribution_delta()[0].size == 0
        for w in range(cut, len(recs)):
            lo = w * W
            b.fold_window(src[lo:lo + W], dst[lo:lo + W], add[lo:lo + W])
            check(b, recs[w])


def test_degree_distribution_state_round_trip():
    e = np.asarray(KAT["degree_distribution_zero"]["events"], dtype=np.int64)
    whole = list(DegreeDistribution(window_edges=2, dense_degrees=4).run(SimpleEdgeStream(e[:, 0], e[:, 1], events=e[:, 2])))
    dd = DegreeDistribution(window_edges=2, dense_degrees=4)
    it = dd.run(SimpleEdgeStream(e[:4, 0], e[:4, 1], events=e[:4, 2]))
    first = [next(it), next(it)]
    state = dd.snapshotState()
    it.close()
    dd2 = DegreeDistribution(window_edges=2, dense_degrees=4, vertex_capacity=5)
    dd2.restoreState(state)
    rest = list(dd2.run(SimpleEdgeStream(e[4:, 0], e[4:, 1], events=e[4:, 2])))
    assert first + rest == whole


# ---- 8. the handle's own stream and torch device inputs ----
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("id_bits", [32, 64])
def test_device_inputs_are_ordered_after_torch(id_bits, path):
    import torch
    nv, n, W, p = 1000, 20000, 257, 0.5
    src, dst, add, recs, _ = _stream_and_oracle(nv, n, W, p)
    dt = torch.int32 if id_bits == 32 else torch.int64
    with DegreeSummary(nv, id_bits=id_bits, path=path, dense_degrees=4) as ds:      # its own stream
        # the inputs are produced on torch's stream right before the call reads them on the handle's
        big = torch.from_numpy(src.copy()).to("cuda")
        s = (big + 7 - 7).to(dt).contiguous()
        d = (torch.from_numpy(dst.copy()).to("cuda") * 3 // 3).to(dt).contiguous()
        a = (torch.from_numpy(add.copy()).to("cuda").to(torch.int32) > 0).to(torch.uint8).contiguous()
        stats = ds.fold_windows(s, d, W, a)
        assert [{k: int(x[k]) for k in x.dtype.names} for x in stats] == [r["stats"] for r in recs]
        check(ds, recs[-1])
    with DegreeSummary(nv, id_bits=id_bits, path=path, dense_degrees=4, stream=torch.cuda.current_stream()) as ds:
        ds.fold_windows(s, d, W, a)
        check(ds, recs[-1])


def test_default_flags_are_sort_all():
    """Flags 0 and GS_DEG_SORT_ALL are one path (every vertex event sorted); GS_DEG_COUNT sorts only
    the events of at-risk vertices, none in a stream of additions."""
    nv, n, W = 1000, 20000, 257
    src, dst, add, recs, _ = _stream_and_oracle(nv, n, W, 0.5)
    for path, whole in ((None, True), ("sort", True), ("count", False)):
        with DegreeSummary(nv, path=path, dense_degrees=4) as ds:
            ds.fold_windows(src, dst, W, add)
            check(ds, recs[-1])
            pc = ds.path_counts()
            assert pc["windows"] == len(recs) and pc["vertex_events"] == 2 * n
            if whole:
                assert pc["exact_events"] == pc["vertex_events"] and pc["exact_windows"] == pc["windows"]
            else:
                assert 0 < pc["exact_events"] < pc["vertex_events"]
    with DegreeSummary(nv, path="count") as ds:
        ds.fold_windows(src, dst, W)
        assert ds.path_counts()["exact_events"] == 0 and ds.path_counts()["exact_windows"] == 0


# ---- 9. lifecycle ----
def test_lifecycle():
    L = _abi.lib()
    assert L.gs_deg_destroy(None) == _abi.GS_OK
    assert L.gs_deg_fold_window(None, None, None, None, 0) == _abi.GS_ERR_INVALID
    assert L.gs_deg_reset(None) == _abi.GS_ERR_INVALID
    n = ctypes.c_uint64()
    assert L.gs_deg_emit_degrees(None, None, None, 0, ctypes.byref(n)) == _abi.GS_ERR_INVALID
    h = ctypes.c_void_p()
    assert L.gs_deg_create(ctypes.byref(h), 0, 32, 0, 0, 0) == _abi.GS_ERR_INVALID
    assert L.gs_deg_create(ctypes.byref(h), 10, 16, 0, 0, 0) == _abi.GS_ERR_INVALID
    assert L.gs_deg_create(ctypes.byref(h), 10, 32, 0, 16, 0) == _abi.GS_ERR_INVALID
    assert L.gs_deg_create(ctypes.byref(h), 10, 32, 0, _abi.GS_DEG_SORT_ALL | _abi.GS_DEG_COUNT, 0) == _abi.GS_ERR_INVALID
    ds = DegreeSummary(10)
    ds.fold_window(np.array([1]), np.array([2]))
    ds.close()
    ds.close()
    with pytest.raises(RuntimeError):
        ds.stats()
    with pytest.raises(ValueError):
        DegreeSummary(10, direction="both")
