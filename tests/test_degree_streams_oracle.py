"""CPU: the vectorised window fold (tests/degree_streams.py) equals WindowOracle after every
window in all three directions, and each structured family meets the input condition it exists
for (event counts past one grid trip, touched and at-risk vertices, the hub's degrees at the
cuts, runs that clamp)."""
import numpy as np
import pytest

import degree_streams as dg
from degrees_oracle import ALL, IN, OUT, WindowOracle, random_events, record

STREAMS = [(3, 40, 1, 0.5), (8, 200, 7, 0.5), (40, 610, 150, 0.5), (40, 610, 150, 0.9), (1000, 20000, 257, 0.5),
           (1000, 20000, 257, 1.0)]


@pytest.mark.parametrize("dirs", [ALL, OUT, IN])
@pytest.mark.parametrize("nv,n,W,p", STREAMS)
def test_fold_vec_equals_the_window_oracle(nv, n, W, p, dirs):
    src, dst, add = random_events(nv, n, p, seed=31 * nv + n + int(10 * p))
    orc = WindowOracle(nv, dirs)
    deg = np.zeros(nv, dtype=np.int64)
    risk = clamped = 0
    for lo in range(0, n, W):
        s, d, a = src[lo:lo + W], dst[lo:lo + W], add[lo:lo + W]
        want = orc.fold(s, d, a)
        f = dg.fold_vec(deg, s, d, None if p == 1.0 else a, dirs)
        np.testing.assert_array_equal(f.deg, orc.deg)
        assert record(f.deg, deg) == want
        arr = record(f.deg, deg, arrays=True)
        assert {k: (v if k == "stats" else (v[0].tolist(), v[1].tolist())) for k, v in arr.items()} == want
        risk += int(f.risk.sum())
        clamped += int(f.clamped.sum())
        assert not np.any(f.clamped & ~f.risk)
        deg = f.deg
    assert (risk, clamped) == (orc.risk_windows, orc.clamped)
    if (nv, p) == (1000, 0.5):
        assert clamped > 1000                              # (4,178 clamped vertex-windows with dirs = ALL)
    if p == 1.0:
        assert risk == 0


def test_fold_vec_small_cases():
    z = np.zeros(4, dtype=np.int64)
    f = dg.fold_vec(z, [2, 2, 2], [2, 1, 1], [False, True, False])       # 2: -1 -1 +1 -1; 1: +1 -1
    assert f.deg.tolist() == [0, 0, 0, 0] and f.touched.tolist() == [1, 2]
    assert f.risk.tolist() == [True, True] and f.clamped.tolist() == [False, True] and f.longest_run == 4
    f = dg.fold_vec(np.array([0, 3, 0, 0]), [1, 1], [2, 2], [False, True], OUT)
    assert f.deg.tolist() == [0, 3, 0, 0] and not f.risk.any()
    f = dg.fold_vec(z, [], [])
    assert f.deg.tolist() == [0, 0, 0, 0] and f.touched.size == 0
    assert z.tolist() == [0, 0, 0, 0]                                    # the input vector is left alone


def test_wide_events():
    src, dst, add, cap = dg.wide_events()
    assert cap == (1 << 20) + 3 and src.size == (1 << 21) + (1 << 19) + 77
    assert src.size > dg.COUNT_SPAN and 2 * src.size > dg.GRID_SPAN      # second trips, k_deg_count's tile loop included
    assert cap % 32 == 3                                                 # vertex capacity - 1 sits in a partial bitmap word
    assert 0.59 < add.mean() < 0.61 and np.any(src == dst)
    (rec,), (f,) = dg.wide_events_reference(False)
    assert f.touched.size > 524288 == dg.GRID_SPAN                       # the touched list takes a second trip
    assert int(f.risk.sum()) > 1000 and int(f.clamped.sum()) > 1000
    assert f.touched[0] == 0 and f.touched[-1] == cap - 1
    assert f.risk[[0, -1]].all() and f.clamped[[0, -1]].all()            # both ends of the id range clamp
    assert int((~f.risk).sum()) > 1000                                   # ... and others take the plain sum
    assert rec["stats"]["n_vertices"] > 524288
    recs, folds = dg.wide_events_reference(True)
    assert len(recs) == 6 and folds[0].clamped[0] and folds[0].touched[0] == 0
    assert folds[2].touched[-1] == cap - 1 and folds[2].clamped[-1]      # event 2^20 + 100 is in window 2
    assert all(int(x.risk.sum()) > 0 for x in folds)
    assert recs[-1]["stats"] == rec["stats"]                             # a window cut changes no degree


def test_hub_ladder():
    windows, cap = dg.hub_ladder()
    recs, folds = dg.hub_ladder_reference()
    assert cap == (1 << 18) + 5 and len(windows) == 10
    hub, hub2 = dg.LADDER_HUB, dg.LADDER_HUB2
    degs = []
    deg = np.zeros(cap, dtype=np.int64)
    for rec in recs:
        deg[:] = 0
        deg[rec["degrees"][0]] = rec["degrees"][1]
        degs.append((int(deg[hub]), int(deg[hub2]), rec["stats"]["max_degree"]))
    assert tuple(d[0] for d in degs[:9]) == dg.LADDER_DEGREES == (1023, 1024, 65535, 65536, 135536, 135536, 65535, 1000, 0)
    assert dg.LDS_DEG == 1024 and dg.DENSE == 65536
    assert [d[1] for d in degs] == [0] * 5 + [40000] * 5
    assert [d[2] for d in degs] == [1023, 1024, 65535, 65536, 135536, 135536, 65535, 40000, 40000, 40000]
    assert windows[4][0].size == 70000 and [w[2] is None for w in windows] == [True] * 6 + [False] * 4
    assert max(int(max(w[0].max(), w[1].max())) for w in windows) == cap - 1
    # window 8: 1,001 deletions at a hub of degree 1,000
    i = int(np.searchsorted(folds[8].touched, hub))
    assert folds[8].touched[i] == hub and folds[8].risk[i] and folds[8].clamped[i]
    # the last window: 200,000 steps at the hub, 0 reached inside the run and at its end
    s, d, a = windows[9]
    assert s.size == 200000 and np.all((s == hub) ^ (d == hub))
    x, zeros, clamps = 0, 0, 0
    for step in np.where(a, 1, -1).tolist():
        clamps += x + step < 0
        x = max(x + step, 0)
        zeros += x == 0
    assert x == 0 == degs[9][0] and zeros >= 4 + clamps and clamps == 10 + 3 + 7
    i = int(np.searchsorted(folds[9].touched, hub))
    assert folds[9].risk[i] and folds[9].clamped[i] and folds[9].longest_run == 200000


@pytest.mark.parametrize("direction", ["out", "all"])
def test_two_long_runs(direction):
    windows, cap, dirs = dg.two_long_runs(direction)
    recs, folds = dg.two_long_runs_reference(direction)
    assert cap == 70001 and cap % 32 == 17 and dirs == {"out": OUT, "all": ALL}[direction]
    s, d, a = windows[0]
    assert s.size == 300000 and np.all(s[0::2] == dg.TWO_U) and np.all(s[1::2] == dg.TWO_W)
    assert dg.TWO_U == cap - 1
    per = 150000 * (2 if direction == "all" else 1)
    assert folds[0].longest_run == per
    for f in folds:
        i, j = (int(np.searchsorted(f.touched, v)) for v in (dg.TWO_W, dg.TWO_U))
        assert f.touched[i] == dg.TWO_W and f.touched[j] == dg.TWO_U
        assert f.risk[i] and f.risk[j]
        if f is folds[0]:                                  # from degree 0 a walk with p = 0.5 clamps at once
            assert f.clamped[i] and f.clamped[j]
    assert all(int(np.sum(r["degrees"][1])) > 0 for r in recs)         # the second window starts above 0
    # the oracle's per-event loop on the first window agrees
    orc = WindowOracle(cap, dirs)
    orc.fold(s, d, a)
    np.testing.assert_array_equal(orc.deg, folds[0].deg)
