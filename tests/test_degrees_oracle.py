"""CPU: the degree oracles (tests/degrees_oracle.py). The restated reference reproduces the
reference's five known answers; the windowed composition oracle equals it after every window on
random event streams, deletions below zero included; the plain sum holds wherever a vertex is not
at risk; the checksum formula is pinned."""
import collections
import functools
import json
import os

import numpy as np
import pytest

from degrees_oracle import (ALL, IN, OUT, ReferenceDistribution, WindowOracle, checksum, checksum_arrays, pair_mix, random_events,
                            reference_degrees, reference_distribution)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KAT = json.load(open(os.path.join(GOLD, "degrees_kat.json")))


def multiset(lines):
    return collections.Counter(tuple(x) for x in lines)


@pytest.mark.parametrize("name", ["degree_distribution", "degree_distribution_zero"])
def test_reference_distribution_known_answers(name):
    k = KAT[name]
    records, per, ref = reference_distribution(k["events"])
    assert multiset(records) == multiset(k["expected"])
    assert records == [tuple(x) for x in k["expected"]]          # (with one subtask the order is the stream's too)
    assert len(per) == len(k["events"])


def test_delete_below_zero_is_ignored():
    _, per, ref = reference_distribution(KAT["degree_distribution_zero"]["events"])
    assert per[-1] == [(1, 1)]                 # "2 3 -": vertex 2 is absent (ignored), vertex 3 leaves: count[1] 2 -> 1
    assert ref.verticesWithDegrees == {1: 1, 4: 2}
    assert ref.distribution() == {1: 1, 2: 1}


@pytest.mark.parametrize("name,cin,cout", [("degrees", True, True), ("in_degrees", True, False), ("out_degrees", False, True)])
def test_reference_get_degrees_known_answers(name, cin, cout):
    k = KAT["get_degrees"]
    records, per, local = reference_degrees(k["edges"], cin, cout)
    assert multiset(records) == multiset(k[name])


FAMILIES = [(nv, p, w) for nv in (3, 8, 40, 1000) for p in (0.5, 0.8, 0.95, 1.0) for w in (1, 7, 64, 300)]


@functools.lru_cache(maxsize=None)
def _run(nv, p, w):
    """(b) against (a) after every window; returns (b)'s counters."""
    n = {3: 300, 8: 600, 40: 1500, 1000: 6000}[nv]
    src, dst, add = random_events(nv, n, p, seed=1000 * nv + int(100 * p) + w)
    ref = ReferenceDistribution()
    orc = WindowOracle(nv)
    for lo in range(0, n, w):
        s, d, a = src[lo:lo + w], dst[lo:lo + w], add[lo:lo + w]
        for x, y, z in zip(s.tolist(), d.tolist(), a.tolist()):
            ref.event(x, y, z)
        rec = orc.fold(s, d, a)
        want_v = sorted(ref.verticesWithDegrees.items())
        assert list(zip(*rec["degrees"])) == want_v
        assert list(zip(*rec["distribution"])) == sorted(ref.distribution().items())
        assert rec["stats"]["checksum"] == checksum(ref.verticesWithDegrees)
        assert rec["stats"]["n_vertices"] == len(want_v)
    return orc


@pytest.mark.parametrize("nv,p,w", FAMILIES)
def test_window_oracle_equals_the_reference(nv, p, w):
    orc = _run(nv, p, w)
    assert orc.plain_sum_broken == 0           # the plain sum holds wherever a vertex is not at risk
    assert orc.vertex_windows > 0
    if p == 1.0:
        assert orc.risk_windows == 0


@pytest.mark.parametrize("nv,p", [(nv, p) for nv in (3, 8, 40, 1000) for p in (0.5, 0.8, 0.95)])
def test_deletion_families_clamp_and_do_not(nv, p):
    """Every family with deletions has at-risk vertex-windows whose clamped result differs from the
    plain sum, and at-risk ones whose result does not (summed over its window sizes)."""
    orcs = [_run(nv, p, w) for w in (1, 7, 64, 300)]
    assert sum(o.clamped for o in orcs) > 0
    assert sum(o.risk_unclamped for o in orcs) > 0


def test_delta_records_are_the_last_record_of_a_changed_key():
    """The window deltas = the reference's last record per key within the window, for keys whose
    value after the window differs from before it."""
    nv, n, w = 8, 400, 7
    src, dst, add = random_events(nv, n, 0.7, seed=5)
    ref = ReferenceDistribution()
    orc = WindowOracle(nv)
    for lo in range(0, n, w):
        before = ref.distribution()
        last = {}
        for x, y, z in zip(src[lo:lo + w].tolist(), dst[lo:lo + w].tolist(), add[lo:lo + w].tolist()):
            for d, c in ref.event(x, y, z):
                last[d] = c
        after = ref.distribution()
        want = sorted((d, c) for d, c in last.items() if before.get(d, 0) != after.get(d, 0))
        rec = orc.fold(src[lo:lo + w], dst[lo:lo + w], add[lo:lo + w])
        assert list(zip(*rec["distribution_delta"])) == want


def test_directions_and_self_loops():
    for dirs, want in ((ALL, 2), (IN, 1), (OUT, 1)):
        o = WindowOracle(4, dirs)
        rec = o.fold([2], [2], [True])
        assert rec["degrees"] == ([2], [want])
    o = WindowOracle(4, OUT)
    assert o.fold([1, 1], [2, 3])["degrees"] == ([1], [2])
    o = WindowOracle(4, IN)
    assert o.fold([1, 1], [2, 3])["degrees"] == ([2, 3], [1, 1])


def test_checksum_formula_is_pinned():
    # splitmix64(v ^ splitmix64(degree ^ 0xD1B54A32D192ED03)), worked out step by step from the definition
    assert pair_mix(0, 1) == 10585070088600740897
    assert pair_mix(1, 1) == 15522800604610918147
    assert checksum({1: 2, 2: 1, 3: 1}) == 12816741179291486377
    assert checksum({}) == 0 == checksum_arrays([], [])
    assert checksum_arrays([1, 2, 3], [2, 1, 1]) == 12816741179291486377
    big = {v: (v * 7919) % 1000 + 1 for v in range(0, 5000, 3)}
    big[4294967294] = 4294967295
    assert checksum_arrays(list(big), list(big.values())) == checksum(big)
