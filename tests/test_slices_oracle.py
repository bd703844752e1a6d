"""CPU: the two restatements of the neighbourhood slice (tests/slices_oracle.py) reproduce the
reference's nine known answers (tests/golden/slice_kat.json: the edges of
GraphStreamTestUtils.getLongLongEdges and the expected lines of TestSlice.java) and agree with each
other on the seeded streams the GPU tests use."""
import json
import os

import numpy as np
import pytest

import slice_streams as S
import slices_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "slice_kat.json")))
EDGES = np.array(KAT["edges"], dtype=np.int64)
SRC, DST, VAL = EDGES[:, 0], EDGES[:, 1], EDGES[:, 2]


def _label(total):
    return "big" if total > KAT["apply_threshold"] else "small"


def kat_lines(case, reduce_fn, rows_fn):
    """The lines a KAT case expects, computed through reduce_fn(direction, op) -> [(v, x)] and
    rows_fn(direction) -> (vertices, offsets, neighbours, values)."""
    d = case["direction"]
    if case["operator"] == "reduce":
        return ["%d,%d" % (v, x) for v, x in reduce_fn(d, "sum")]
    v, o, nb, x = rows_fn(d)
    out = []
    for r in range(len(v)):
        row = [int(t) for t in x[int(o[r]):int(o[r + 1])]]
        if case["operator"] == "fold":                  # SumEdgeValues: accum.f1 + edgeValue from (0, 0)
            acc = 0
            for t in row:
                acc = O.wrap(acc + t)
            out.append("%d,%d" % (int(v[r]), acc))
        else:                                           # SumEdgeValuesApply
            out.append("%d,%s" % (int(v[r]), _label(sum(row))))
    return out


def test_kat_file_has_the_nine_cases():
    assert len(KAT["edges"]) == 7 and len(KAT["cases"]) == 9
    assert sorted({c["operator"] for c in KAT["cases"]}) == ["apply", "fold", "reduce"]


@pytest.mark.parametrize("case", KAT["cases"], ids=[c["name"] for c in KAT["cases"]])
def test_reference_rule_reproduces_kat(case):
    got = kat_lines(case, lambda d, op: O.reference_reduce(O.reference_rows(SRC, DST, VAL, d), op),
                    lambda d: O.reference_csr(O.reference_rows(SRC, DST, VAL, d)))
    assert sorted(got) == sorted(case["expected"])


@pytest.mark.parametrize("case", KAT["cases"], ids=[c["name"] for c in KAT["cases"]])
def test_numpy_reproduces_kat(case):
    got = kat_lines(case, lambda d, op: list(zip(*[a.tolist() for a in O.numpy_reduce(SRC, DST, VAL, d, op)])),
                    lambda d: O.numpy_csr(SRC, DST, VAL, d))
    assert sorted(got) == sorted(case["expected"])


def agree(src, dst, val):
    for d in O.DIRECTIONS:
        rows = O.reference_rows(src, dst, val, d)
        for op in O.OPS:
            v, x = O.numpy_reduce(src, dst, val, d, op)
            assert O.reference_reduce(rows, op) == list(zip(v.tolist(), x.tolist())), (d, op)
            assert O.reference_stats(rows, op) == O.numpy_stats(src, dst, val, d, op), (d, op)
        rv, ro, rn, rx = O.reference_csr(rows)
        nv, no, nn, nx = O.numpy_csr(src, dst, val, d)
        assert (rv, ro, rn, rx) == (nv.tolist(), no.tolist(), nn.tolist(), nx.tolist()), d


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 4097])
def test_oracles_agree_on_random_streams(n):
    for s, d, x, _ in (S.rmat(12, n, 100 + n), S.uniform(5, n, 200 + n), S.uniform(4097, n, 300 + n),
                       S.uniform((1 << 21) + 1, n, 400 + n)):
        agree(s, d, x)


@pytest.mark.parametrize("name", sorted(S.value_cases()))
def test_oracles_agree_on_value_cases(name):
    s, d, x, _ = S.value_cases()[name]
    agree(s, d, x)


def test_oracles_agree_on_structured_streams():
    for s, d, x, _ in (S.row_shapes(), S.row_shapes(63), S.tile_seams(), S.distinct(1000), S.hub(5000),
                       S.hub_and_singles(5000, 100), S.two_hubs(5000)):
        agree(s, d, x)
    s, d, x, _, _ = S.multi_window(3, 100, 7)
    agree(s, d, x)


def test_row_shapes_have_the_lengths_they_name():
    s, d, x, _ = S.row_shapes(5)
    rows = O.reference_rows(s, d, x, "out")
    assert [len(rows[k]) for k in sorted(rows)] == [5] + list(S.ROW_LENGTHS)
    assert np.any(np.diff(s) < 0)                       # arrival order is not sorted order
    s, d, x, _ = S.hub()
    assert len(O.reference_rows(s, d, x, "out")) == 1 and s.size == S.HUB_EDGES >= 8 * S.TILE


def test_first_and_last_depend_on_arrival_order():
    s, d, x, _ = S.value_cases()["repeated_edges"]
    rows = O.reference_rows(s, d, x, "out")
    assert dict(O.reference_reduce(rows, "first"))[1] == 30 and dict(O.reference_reduce(rows, "last"))[1] == 15
    assert dict(O.reference_reduce(rows, "min"))[1] == 10


def test_self_loop_entries():
    s, d, x, _ = S.value_cases()["self_loops"]
    assert dict(O.reference_reduce(O.reference_rows(s, d, x, "all"), "count"))[1] == 4     # two loops at 1, twice each
    assert dict(O.reference_reduce(O.reference_rows(s, d, x, "out"), "count"))[1] == 2
    assert dict(O.reference_reduce(O.reference_rows(s, d, x, "in"), "count"))[1] == 2


def test_sum_wraps_as_java_long():
    s, d, x, _ = S.value_cases()["wrap_up"]
    assert dict(O.reference_reduce(O.reference_rows(s, d, x, "out"), "sum"))[1] == O.wrap(2 * S.I64_MAX + 5) == 3
    s, d, x, _ = S.value_cases()["wrap_down"]
    assert dict(O.reference_reduce(O.reference_rows(s, d, x, "out"), "sum"))[1] == -5


def test_checksum_forms_agree():
    g = np.random.default_rng(7)
    v = g.integers(0, 1 << 32, size=500, dtype=np.int64)
    x = S.values(500, 8)
    assert O.checksum(zip(v.tolist(), x.tolist())) == O.checksum_arrays(v, x)
    assert O.checksum([]) == O.checksum_arrays([], []) == 0
    # the library's mixing, as restated for the degree summary
    import degrees_oracle
    assert O.checksum([(5, 9)]) == degrees_oracle.pair_mix(5, 9)


def test_python_binding_names_the_slice():
    """The feature's public surface exists (this fails on a tree without it)."""
    import gsgpu
    from gsgpu import _abi
    assert hasattr(gsgpu, "SnapshotStream")
    assert {"gs_slice_window", "gs_slice_reduce", "gs_slice_rows", "gs_slice_reduce_windows"} <= set(_abi.EXPORTED_SYMBOLS)
    st = gsgpu.SimpleEdgeStream(SRC, DST, values=VAL)
    assert st.values.tolist() == VAL.tolist() and gsgpu.SimpleEdgeStream(SRC, DST).values is None
