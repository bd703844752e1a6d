"""GPU parity of the streaming degrees (gs_deg_*) on the structured families of
tests/degree_streams.py against its vectorised fold: 21 vertex bits and an odd capacity, windows
of more than one grid trip, the default dense cut and the LDS cut of the distribution, runs of
hundreds of thousands of steps at one vertex with clamps inside. Every case runs the sorting path
and the counting path (GS_DEG_COUNT). Integer path: every comparison is exact."""
import numpy as np
import pytest

import degree_streams as dg
from gsgpu import DegreeSummary

pytestmark = pytest.mark.gpu

PATHS = ["sort", "count"]
STAT_KEYS = ("n_vertices", "n_degrees", "max_degree", "checksum")


def _pairs_equal(got, want):
    k, v = got
    assert k.size == want[0].size
    np.testing.assert_array_equal(k.astype(np.int64), want[0])
    np.testing.assert_array_equal(v.astype(np.int64), want[1])


def _find_ids(rec, cap, seed):
    """64 ids: both ends of the id range, vertices with a degree, vertices the window changed, others."""
    rng = np.random.default_rng(seed)
    pools = [rec["degrees"][0], rec["degrees_delta"][0], np.arange(cap)]
    ids = [np.array([0, cap - 1], dtype=np.int64)]
    for p, k in zip(pools, (30, 16, 16)):
        ids.append(p[rng.integers(0, p.size, size=k)].astype(np.int64) if p.size else np.zeros(k, dtype=np.int64))
    return np.concatenate(ids)


def check(ds, rec, cap, seed=0):
    """The handle's summary equals the reference's record of the same window."""
    assert ds.stats() == rec["stats"]
    _pairs_equal(ds.degrees(), rec["degrees"])
    _pairs_equal(ds.degrees_delta(), rec["degrees_delta"])
    _pairs_equal(ds.distribution(), rec["distribution"])
    _pairs_equal(ds.distribution_delta(), rec["distribution_delta"])
    ids = _find_ids(rec, cap, seed)
    assert ids.size == 64
    deg = np.zeros(cap, dtype=np.int64)
    deg[rec["degrees"][0]] = rec["degrees"][1]
    assert ds.find(ids).tolist() == deg[ids].tolist()


def _stats_list(stats):
    return [{k: int(s[k]) for k in STAT_KEYS} for s in stats]


# ---- wide_events ----
@pytest.mark.parametrize("path,id_bits", [("sort", 32), ("count", 32), ("sort", 64)])
def test_wide_events_one_window(path, id_bits):
    src, dst, add, cap = dg.wide_events()
    (rec,), _ = dg.wide_events_reference(False)
    with DegreeSummary(cap, id_bits=id_bits, path=path) as ds:
        ds.fold_window(src, dst, add)
        check(ds, rec, cap)
        pc = ds.path_counts()
        assert pc["windows"] == 1 and pc["vertex_events"] == 2 * src.size and pc["exact_windows"] == 1
        if path == "count":
            assert 0 < pc["exact_events"] < pc["vertex_events"]          # the exact path ran, on the at-risk vertices' events
        else:
            assert pc["exact_events"] == pc["vertex_events"]


@pytest.mark.parametrize("path", PATHS)
def test_wide_events_window_by_window(path):
    src, dst, add, cap = dg.wide_events()
    recs, _ = dg.wide_events_reference(True)
    W = dg.WIDE_WINDOW
    with DegreeSummary(cap, id_bits=32, path=path) as ds:
        for w, rec in enumerate(recs):
            ds.fold_window(src[w * W:(w + 1) * W], dst[w * W:(w + 1) * W], add[w * W:(w + 1) * W])
            check(ds, rec, cap, seed=w)


@pytest.mark.parametrize("path", PATHS)
def test_wide_events_fold_windows(path):
    src, dst, add, cap = dg.wide_events()
    recs, _ = dg.wide_events_reference(True)
    with DegreeSummary(cap, id_bits=32, path=path) as ds:
        stats = ds.fold_windows(src, dst, dg.WIDE_WINDOW, add)
        assert _stats_list(stats) == [r["stats"] for r in recs]
        check(ds, recs[-1], cap)
        pc = ds.path_counts()
        assert pc["windows"] == len(recs) == pc["exact_windows"]
        if path == "count":
            assert 0 < pc["exact_events"] < pc["vertex_events"]


@pytest.mark.parametrize("path", PATHS)
def test_wide_events_from_device_tensors(path):
    import torch
    src, dst, add, cap = dg.wide_events()
    recs, _ = dg.wide_events_reference(True)
    # the inputs are produced on torch's stream right before the call reads them on the handle's
    s = (torch.from_numpy(src.copy()).to("cuda") + 7 - 7).to(torch.int32).contiguous()
    d = (torch.from_numpy(dst.copy()).to("cuda") * 3 // 3).to(torch.int32).contiguous()
    a = torch.from_numpy(add.copy()).to("cuda").to(torch.uint8).contiguous()
    with DegreeSummary(cap, id_bits=32, path=path) as ds:
        stats = ds.fold_windows(s, d, dg.WIDE_WINDOW, a)
        assert _stats_list(stats) == [r["stats"] for r in recs]
        check(ds, recs[-1], cap)


# ---- hub_ladder ----
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("id_bits", [32, 64])
def test_hub_ladder(id_bits, path):
    """The default dense cut: the hub's count moves from LDS to the dense array at 1,024, to the
    sparse table at 65,536, and back; the maximum is rescanned when the hub falls below the second."""
    windows, cap = dg.hub_ladder()
    recs, folds = dg.hub_ladder_reference()
    with DegreeSummary(cap, id_bits=id_bits, path=path) as ds:
        for w, ((src, dst, add), rec) in enumerate(zip(windows, recs)):
            ds.fold_window(src, dst, add)
            check(ds, rec, cap, seed=w)
            if w < 9:
                assert ds.find([dg.LADDER_HUB]).tolist() == [dg.LADDER_DEGREES[w]]
            if w == 5 and path == "count":
                pc = ds.path_counts()                                    # additions only so far: nothing was sorted
                assert pc["windows"] == 6 and pc["exact_windows"] == 0 and pc["exact_events"] == 0
        if path == "count":
            pc = ds.path_counts()
            at_risk = [bool(f.risk.any()) for f in folds]
            assert at_risk == [False] * 8 + [True] * 2                   # (deletions a degree covers put no vertex at risk)
            assert pc["windows"] == 10 and pc["exact_windows"] == sum(at_risk)


# ---- two_long_runs ----
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("direction", ["out", "all"])
def test_two_long_runs(direction, path):
    windows, cap, _ = dg.two_long_runs(direction)
    recs, _ = dg.two_long_runs_reference(direction)
    with DegreeSummary(cap, id_bits=32, direction=direction, path=path) as ds:
        for w, ((src, dst, add), rec) in enumerate(zip(windows, recs)):
            ds.fold_window(src, dst, add)
            check(ds, rec, cap, seed=w)
