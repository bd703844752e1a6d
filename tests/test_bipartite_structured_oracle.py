"""CPU checks of tests/bipartite_streams.py: the double-cover reference against the oracle's
union-find with parity and its BFS 2-colouring (oracle/bipartite.py), closed forms as a second
witness, and the input conditions tests/test_gpu_bipartite_structured.py depends on."""
import numpy as np
import pytest

import bipartite_streams as bs
from bipartite import ParityUnionFind, bfs_bipartition

SMALL = bs.L_SMALL
# the window (0-based) in which each failing family fails at full size: an input condition of the
# GPU tests, named by the reference and recorded here
FAIL_WINDOW = {"odd_cycle": 8, "odd_cycle_mid": 3, "chord_first": 5, "grid_diag": 7}


def _as_dicts(ref):
    v, k, s = ref.pairs()
    return ref.ok, dict(zip(v.tolist(), k.tolist())), dict(zip(v.tolist(), s.tolist()))


@pytest.mark.parametrize("name", bs.FAMILIES)
def test_reference_vs_union_find_small_every_window(name):
    st = bs.stream(name, SMALL)
    refs = bs.reference_windows(name, None, SMALL)
    assert len(refs) == bs.n_windows(name, SMALL)
    uf = ParityUnionFind()
    s, d = st.src.tolist(), st.dst.tolist()
    for w, ref in enumerate(refs):
        for i in range(w * st.W, min((w + 1) * st.W, len(s))):
            uf.union(s[i], d[i])
        assert _as_dicts(ref) == uf.emission(), "window %d" % w
    assert _as_dicts(refs[-1]) == bfs_bipartition(st.src, st.dst)


@pytest.mark.parametrize("name", bs.FAMILIES)
def test_reference_vs_union_find_full_size_final(name):
    """Every family at full size: the final state, and for the failing families the window in which
    the union-find first sees the odd cycle, equal the reference's. (The Python union-find takes
    0.4 s to 2 s per family, Q18's 2.4 M edges 6 s to 12 s.)"""
    st = bs.stream(name)
    uf = ParityUnionFind()
    failed_at = None
    for i, (a, b) in enumerate(zip(st.src.tolist(), st.dst.tolist())):
        uf.union(a, b)
        if failed_at is None and not uf.ok:
            failed_at = i
    ok, key, sign = uf.emission()
    ref = bs.reference_windows(name)[-1]
    assert ref.ok == ok == (name not in bs.FAILING)
    assert bs.first_failed_window(name) == (None if failed_at is None else failed_at // st.W)
    v, k, s = ref.pairs()
    assert v.size == len(key)
    if ok:
        assert ref.status == (True, len(key), len(set(key.values())))
        assert np.array_equal(k, np.array([key[x] for x in v.tolist()]))
        assert np.array_equal(s, np.array([sign[x] for x in v.tolist()]))


@pytest.mark.parametrize("L", [SMALL, bs.L_FULL])
def test_input_conditions(L):
    full = L == bs.L_FULL
    nb = L + 3
    for name in bs.FAMILIES:
        oks = [r.ok for r in bs.reference_windows(name, None, L)]
        if name not in bs.FAILING:
            assert all(oks), name
            continue
        w = bs.first_failed_window(name, L)
        assert w is not None and all(oks[:w]) and not any(oks[w:]), name
        st = bs.stream(name, L)
        if name == "odd_cycle":
            assert w == len(oks) - 1
        else:                                   # a full-size window, not the first, not the last
            assert 0 < w < len(oks) - 1 and (w + 1) * st.W <= st.src.size, name
        if name == "odd_cycle_mid":
            assert w == 3
        if full:
            assert w == FAIL_WINDOW[name], name
        for r in bs.reference_windows(name, None, L)[w:]:
            assert r.status == (False, 0, 0) and r.pairs()[0].size == 0 and r.string() == "(false,{})"
    final = {name: bs.reference_windows(name, None, L)[-1] for name in bs.FAMILIES}
    assert final["matching_loops"].status == (True, nb, L // 2 + 3)
    for name in ("asc_path", "desc_path", "shuffled_path", "star_max_hub"):
        assert final[name].status == (True, nb, 1), name
    assert final["complete_bipartite"].status == (True, 2 * bs.stream("complete_bipartite", L).info["m"], 1)
    assert final["hypercube"].status == (True, L, 1)
    assert final["grid"].status == (True, L, 1)
    assert final["even_cycle"].status == (True, nb - 1, 1)
    st = bs.stream("even_cycle", L)
    assert final["even_cycle"].pairs()[0].size == nb - 1 and st.perm[nb - 1] not in final["even_cycle"].pairs()[0]
    if full:
        assert (nb, bs.WB) == (bs.NB, bs.stream("asc_path").W) == ((1 << 18) + 3, 1 << 15)
        assert bs.stream("hypercube").cap == 1 << 18 and bs.stream("rmat_sides").cap == 1 << 17
        assert bs.stream("rmat_sides").W == 1 << 16 and bs.n_windows("rmat_sides") == 16
        st = bs.stream("grid_diag")
        assert st.info["diag_at"] == 6 * bs.WB - 1


def _position(perm, n):
    pos = np.full(perm.size, -1, dtype=np.int64)
    pos[perm[:n]] = np.arange(n)
    return pos


@pytest.mark.parametrize("L", [SMALL, bs.L_FULL])
def test_closed_forms(L):
    nb = L + 3
    for name in ("asc_path", "desc_path"):
        v, k, s = bs.reference_windows(name, None, L)[-1].pairs()
        assert np.array_equal(v, np.arange(nb)) and not k.any() and np.array_equal(s, v % 2 == 0)
    for name, n in (("shuffled_path", nb), ("even_cycle", nb - 1)):
        st = bs.stream(name, L)
        v, k, s = bs.reference_windows(name, None, L)[-1].pairs()
        pos = _position(st.perm, n)
        assert np.array_equal(v, np.sort(st.perm[:n])) and np.all(k == v[0])
        assert np.array_equal(s, (pos[v] - pos[v[0]]) % 2 == 0)
    v, k, s = bs.reference_windows("hypercube", None, L)[-1].pairs()
    assert np.array_equal(v, np.arange(L)) and not k.any()
    assert np.array_equal(s, bs.hypercube_sign(L))
    st = bs.stream("grid", L)
    v, k, s = bs.reference_windows("grid", None, L)[-1].pairs()
    pos = _position(st.perm, L)                                   # row-major id of a label
    m = st.info["m"]
    rc = pos // m + pos % m
    assert np.all(k == v[0]) and np.array_equal(s, (rc[v] - rc[v[0]]) % 2 == 0)
    for ref in bs.reference_windows("rmat_sides", None, L):
        v, k, s = ref.pairs()
        assert ref.ok and np.array_equal(s, (v & 1) == (k & 1))


def test_checksum_is_the_suite_formula():
    """bs.checksum equals test_gpu_bipartite._checksum's formula, written out per vertex."""
    from pyoracle import _np_splitmix64
    ref = bs.reference_windows("matching_loops", None, bs.L_TINY)[-1]
    v, k, s = ref.pairs()
    lab = np.array([(int(a) << 1) | (1 if b else 0) for a, b in zip(k, s)], dtype=np.uint64)
    mix = _np_splitmix64(v.astype(np.uint64) ^ _np_splitmix64(lab ^ np.uint64(0xD1B54A32D192ED03)))
    with np.errstate(over="ignore"):
        assert ref.checksum == int(np.sum(mix, dtype=np.uint64))
    assert bs.checksum(v[:0], k[:0], s[:0]) == 0


def test_staging_stream_is_the_connected_hypercube():
    """tests/test_gpu_bipartite_structured.py compares this stream's final state with the closed
    form of Q18: every vertex present, one component."""
    s, d = bs.staging_stream()
    assert s.size == (1 << 22) + 5
    ok, v, k, sg = bs.cover_reference(s, d, bs.L_FULL)
    assert ok and v.size == bs.L_FULL and not k.any() and np.array_equal(sg, bs.hypercube_sign(bs.L_FULL))


# ---- csrc/bip.hip's bip_find / bip_union restated serially, and two ways to get them wrong ----
def _serial_parity_forest(src, dst, cap, W, mutate=None):
    """One packed word (parent << 1 | parity) per vertex, min-rooted hooks, path halving by min of
    the packed word, as the kernel does it, one edge after another; the state after every window as
    (ok, {v: key}, {v: sign}). mutate "halve": the halving writes wc & 1 instead of (wc ^ wp) & 1;
    "hook": the hook writes pu ^ pv without the required relation."""
    INV = 0xFFFFFFFF
    w = [INV] * cap
    ok = True

    def find(x):
        cur, wc, par = x, w[x], 0
        while True:
            p = wc >> 1
            if p >= cur:
                return cur, par
            wp = w[p]
            par ^= wc & 1
            pp = wp >> 1
            if pp < p:
                bit = (wc & 1) if mutate == "halve" else ((wc ^ wp) & 1)
                w[cur] = min(w[cur], (pp << 1) | bit)
            cur, wc = p, wp

    out = []
    s, d = np.asarray(src).tolist(), np.asarray(dst).tolist()
    for i, (u, v) in enumerate(zip(s, d)):
        for x in (u, v):
            if w[x] == INV:
                w[x] = x << 1
        if u != v:
            (ru, pu), (rv, pv) = find(u), find(v)
            if ru == rv:
                ok = ok and (pu ^ pv) == 1
            else:
                hi, lo = max(ru, rv), min(ru, rv)
                w[hi] = (lo << 1) | ((pu ^ pv) if mutate == "hook" else (pu ^ pv ^ 1))
        if (i + 1) % W == 0 or i + 1 == len(s):
            key, sign = {}, {}
            if ok:
                for x in range(cap):
                    if w[x] != INV:
                        cur, par = x, 0
                        while (w[cur] >> 1) < cur:
                            par ^= w[cur] & 1
                            cur = w[cur] >> 1
                        key[x], sign[x] = cur, par == 0
            out.append((ok, key, sign))
    return out


@pytest.mark.parametrize("name", ["shuffled_path", "odd_cycle"])
def test_reference_catches_a_wrong_parity_forest(name):
    """The serial restatement equals the reference in every window; with the halving's parity or the
    hook's relation wrong it does not (so a kernel wrong in either way fails every GPU test that
    compares this family's windows)."""
    st = bs.stream(name, SMALL)
    want = [_as_dicts(r) for r in bs.reference_windows(name, None, SMALL)]
    assert _serial_parity_forest(st.src, st.dst, st.cap, st.W) == want
    for mutate in ("halve", "hook"):
        got = _serial_parity_forest(st.src, st.dst, st.cap, st.W, mutate)
        assert want[-2][0] and got[-2] != want[-2], mutate      # the last full window: deep trees, still bipartite
