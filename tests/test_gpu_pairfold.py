"""Directed GPU parity of the pair / survivor folds' wave-combined hooks (combine_hooks,
csrc/cc_kernels.hpp:654-703): gs_cc_fold_pairs and gs_cc_fold_pairs32 (k_fold<..., AOS>), the slot
folds of the all-gather and gather exchanges (k_fold_slots, k_fold_slots_sparse) and their marks,
every comparison exact against the C oracle fed the same pairs as one window (the slot folds:
as the window behind a first one that sizes the slots).

What makes lanes combine (cc_kernels.hpp:668-681): every live lane holds its union's two ROOTS,
hi > lo; the first live lane's hi is H, and the lanes with hi == H are combined — so lanes combine
when they share the LARGER root. The batches here are therefore (v_i, R) with R = capacity - 1 (a
fresh vertex, or a root above every root(v_i)) and the v_i in distinct components with smaller
roots: the lane with the smallest root(v_i) = Lmin keeps union(R, Lmin), lanes with the same
root(v_i) drop theirs (:692-695), every other lane's union becomes union(root(v_i), Lmin)
(:696-702). The mirror image (v_i, 0) shares the SMALLER root and must not combine.

The callers reach that function in diverged code — k_fold's `g < groups` (:931, :935),
k_fold_slots' `i < n` (:1526), k_fold_slots_sparse (sparse_ids.hpp:163) — so the pair counts sit on
the lane, wave and workgroup edges of one pair per thread (mature folds of at most 2^22 pairs,
cc_api.hip kSmallPairFold) and of two (young folds, kYoungEpt), where the tail wave is partly
filled; one large batch runs the four-pairs-per-thread instance behind the 1024-pair head launch.

Pre-states (one handle per pre-state and id width, reset() between cases):
  s0  fresh after reset(): the young path (edges since reset < capacity / 4, cc_api.hip
      launch_fold_split), two pairs per thread from the work counter; Lmin and R uninitialised words
  s1  mature, no giant: capacity / 4 edges of 3-vertex paths, closed; members are path tails and
      middles (a walk), roots and untouched ids
  s2  mature, the giant filter on: a path over 60 % of the ids, closed ONCE. Close 0 samples the
      giant itself (compress_impl: force = closes % kPickEvery == 0 && closes == 0 -> k_pick_giant,
      a label held by >= 16 and >= 1/4 of the seen samples) and k_compress writes it to the slot the
      next fold reads, so `*f.giant != kInvalid` from then on. The test sees that the filter is on
      through gs_cc_filter_edges: an edge inside the giant is dropped, one outside survives. Members
      inside the giant (R is then claimed straight under its root, union_group_g<..., RING=false>,
      :790-818) and outside it, below the giant's root (they combine on H = that root) and above.

tests/test_gpu_variants.py::test_pair_fold_switches runs this module again with
GSGPU_PAIR_COMBINE=0 and / or GSGPU_PAIR_HALVE=0 (the library reads them once per process).
"""
import numpy as np
import pytest

from gsgpu import DisjointSet, GsError, _abi
from pyoracle import EMIT_CHECKSUM, _np_splitmix64
from test_gpu_comm import _long_ids, _run_local

pytestmark = pytest.mark.gpu

CAP = 4096
R = CAP - 1
# lane, wave and workgroup (256 threads) edges for one pair per thread and for two
COUNTS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1000]
FAMILIES = 64                                    # ids >= CAP - FAMILIES are kept for the shared roots


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch


def _paths3(first, count):
    """count 3-vertex paths first+3k - first+3k+1 - first+3k+2 (2 edges each), tail edge first."""
    k = first + 3 * np.arange(count, dtype=np.int64)
    return np.concatenate([k + 2, k + 1]), np.concatenate([k + 1, k])


def _round_robin(lists, n):
    out, i = [], 0
    while len(out) < n:
        took = False
        for l in lists:
            if i < len(l) and len(out) < n:
                out.append(l[i])
                took = True
        assert took, "pool exhausted"
        i += 1
    return np.array(out, dtype=np.int64)


class PreState:
    """Edges folded and closed before a batch, and the members a batch may name: pool[zero][:n] are n
    vertices (zero: vertex 0 among them) in distinct components — but for s2's members inside the
    giant, which share one on purpose. root[v] = the label v holds before the batch (v if untouched)."""

    def __init__(self, name, oracle, cap=CAP):
        self.name, self.cap = name, cap
        if name == "s0":
            self.u = self.v = np.empty(0, dtype=np.int64)
            ids = np.random.default_rng(7).permutation(np.arange(1, cap - FAMILIES))
            self.pool = {True: np.concatenate([[0], ids[:999]]), False: ids[:1000]}
        elif name == "s1":
            npaths = cap // 8                                # 2 edges each: capacity / 4 edges
            self.u, self.v = _paths3(0, npaths)
            member = [3 * k + (2, 0, 1)[k % 3] for k in range(npaths)]      # tail, root, middle
            fresh = list(range(3 * npaths, cap - FAMILIES))
            self.pool = {True: _round_robin([[0] + member[1:], fresh], 1000),
                         False: _round_robin([member[1:], fresh], 1000)}
        else:
            g0, g1 = cap // 4, cap // 4 + (cap * 6) // 10    # the giant: a path over [g0, g1)
            gu = np.arange(g0, g1 - 1, dtype=np.int64)
            pu, pv = _paths3(0, 200)
            perm = np.random.default_rng(9).permutation(gu.size)
            self.u, self.v = np.concatenate([gu[perm] + 1, pu]), np.concatenate([gu[perm], pv])
            self.giant = (g0, g1)
            inside = [g0 + 1 + (37 * j) % (g1 - g0 - 1) for j in range(250)]
            member = [3 * k + (2, 0, 1)[k % 3] for k in range(200)]
            below = list(range(600, g0))
            above = list(range(g1, cap - FAMILIES))
            self.pool = {True: _round_robin([[0] + member[1:], inside, below, above], 1000),
                         False: _round_robin([member[1:], inside, below, above], 1000)}
        assert name == "s0" or self.u.size >= cap // 4
        self.labels = np.full(cap, -1, dtype=np.int64)       # the pre-state's emission (-1: untouched)
        if self.u.size:
            self.labels = oracle.run(self.u, self.v, self.u.size, partitions=1, emit=EMIT_CHECKSUM, label_cap=cap,
                                     want_final=True)["final"]
        self.root = np.where(self.labels >= 0, self.labels, np.arange(cap, dtype=np.int64))
        self._dev, self._filter_seen = {}, set()

    def enter(self, torch, ds):
        """reset(), then this pre-state folded and closed."""
        ds.reset()
        if not self.u.size:
            return
        dt = np.int32 if ds.id_bits == 32 else np.int64
        if dt not in self._dev:
            self._dev[dt] = (torch.from_numpy(self.u.astype(dt)).cuda(), torch.from_numpy(self.v.astype(dt)).cuda())
        ds.fold(*self._dev[dt])
        ds.close_window()
        if self.name == "s2" and id(ds) not in self._filter_seen:    # the giant filter is on (module docstring)
            self._filter_seen.add(id(ds))
            g0, g1 = self.giant
            out = torch.empty(4, dtype=torch.int32, device="cuda")
            assert ds.filter_edges(np.array([g0 + 5, 1]).astype(dt), np.array([g1 - 5, 601]).astype(dt), out) == 1
            assert out[:2].tolist() == [1, 601]


@pytest.fixture(scope="module")
def states(oracle):
    return {n: PreState(n, oracle) for n in ("s0", "s1", "s2")}


@pytest.fixture(scope="module")
def handles():
    made = {}

    def get(bits, cap=CAP, marks=False):
        key = (bits, cap, marks)
        if key not in made:
            made[key] = DisjointSet(cap, id_bits=bits, track_marks=marks)
        return made[key]
    yield get
    for ds in made.values():
        ds.close()


def _interleave(bu, bv, dt):
    p = np.empty(2 * len(bu), dtype=dt)
    p[0::2] = bu
    p[1::2] = bv
    return p


def _oracle(oracle, st, bu, bv, cap=None):
    u = np.concatenate([st.u, np.asarray(bu, dtype=np.int64)])
    v = np.concatenate([st.v, np.asarray(bv, dtype=np.int64)])
    return oracle.run(u, v, u.size, partitions=1, emit=EMIT_CHECKSUM, label_cap=cap or st.cap, want_final=True)


def _equal(ds, want):
    """Closed summary vs the oracle: dense labels, and the checksum with its vertex and component
    counts (an Lmin or R left uninitialised, or initialised twice, shows there)."""
    ds.close_window()
    return (ds.checksum() == (int(want["checksums"][0]), want["final_vertices"], want["final_components"])
            and np.array_equal(ds.dense().astype(np.int64), want["final"]))


def _pair_case(torch, oracle, ds, st, bu, bv):
    st.enter(torch, ds)
    dt = np.int32 if ds.id_bits == 32 else np.int64
    ds.fold_pairs(torch.from_numpy(_interleave(bu, bv, dt)).cuda())
    return _equal(ds, _oracle(oracle, st, bu, bv))


def _orders(st, members, rng):
    """Orders of one member set: by the root each lane will hold (ascending, descending), shuffled,
    and shuffled with the smallest root in lane 0, in the last active lane, in the tail wave's middle."""
    n = len(members)
    asc = members[np.lexsort((members, st.root[members]))]
    yield "asc", asc
    yield "desc", asc[::-1]
    sh = members[rng.permutation(n)]
    yield "shuffled", sh
    tail0 = (n - 1) // 64 * 64
    for name, pos in (("min_first", 0), ("min_last", n - 1), ("min_mid", tail0 + (n - 1 - tail0) // 2)):
        a = sh.copy()
        i = int(np.argmin(st.root[a]))
        a[i], a[pos] = a[pos], a[i]
        yield name, a


def _family_a(st, n):
    rng = np.random.default_rng(1000 + n)
    for zero in (True, False):
        members = st.pool[zero][:n]
        for name, m in _orders(st, members, rng):
            yield "%s,%s" % (name, "with0" if zero else "no0"), m
    sh = st.pool[True][:n][rng.permutation(n)]
    yield "twice_adjacent", np.repeat(sh, 2)[:n]           # a non-owner lane with lo == Lmin: its union is the owner's
    yield "twice_64_apart", np.concatenate([np.tile(sh[b:b + 64], 2) for b in range(0, n, 64)])[:n]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("state", ["s0", "s1", "s2"])
def test_one_shared_root(oracle, torch_cuda, states, handles, state, bits):
    """A: n pairs (v_i, R), n on every lane / wave / workgroup edge, in every order of the members."""
    st, ds = states[state], handles(bits)
    bad = []
    if not _pair_case(torch_cuda, oracle, ds, st, [5, 1, 3], [R, R, R]):
        bad.append("(5,R),(1,R),(3,R)")                  # the advisor's example
    for n in COUNTS:
        for name, m in _family_a(st, n):
            assert len(m) == n
            if not _pair_case(torch_cuda, oracle, ds, st, m, np.full(n, R)):
                bad.append("n=%d,%s" % (n, name))
    assert not bad, "%d cases differ from the oracle: %s" % (len(bad), bad[:40])


def _family_b(st, n, K, rng):
    """K shared roots R_f = CAP - 1 - f, their pairs interleaved so every wave holds several H (only
    the first live lane's H group is combined per call; the rest fall through)."""
    m = st.pool[True][:n][rng.permutation(n)]
    f = np.arange(n) % K
    return m, R - f


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("state", ["s0", "s1", "s2"])
def test_several_roots_in_one_wave(oracle, torch_cuda, states, handles, state, bits):
    st, ds = states[state], handles(bits)
    bad = []
    for K in (2, 5, 64):
        for n in (65, 129, 513, 1000):
            rng = np.random.default_rng(2000 + 7 * n + K)
            bu, bv = _family_b(st, n, K, rng)
            if not _pair_case(torch_cuda, oracle, ds, st, bu, bv):
                bad.append("K=%d,n=%d" % (K, n))
            ju = bu.copy()
            ju[:K] = bu[0]                               # one member in every family: all families join
            if not _pair_case(torch_cuda, oracle, ds, st, ju, bv):
                bad.append("K=%d,n=%d,joined" % (K, n))
    for n in (65, 129, 513, 1000):                       # lo shared, hi distinct: nothing to combine
        m = st.pool[False][:n][np.random.default_rng(3000 + n).permutation(n)]
        if not _pair_case(torch_cuda, oracle, ds, st, m, np.zeros(n, dtype=np.int64)):
            bad.append("mirror,n=%d" % n)
    assert not bad, "%d cases differ from the oracle: %s" % (len(bad), bad[:40])


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("state", ["s0", "s1", "s2"])
def test_dead_lanes_among_live_ones(oracle, torch_cuda, states, handles, state, bits):
    """Self-loops, out-of-range ids and already-joined pairs between the live (v_i, R): the dead lanes
    take no part, and the fold reports GS_ERR_RANGE exactly as fold() does for the same edges."""
    torch = torch_cuda
    st, ds = states[state], handles(bits)
    rng = np.random.default_rng(41)
    n = 700
    m = st.pool[True][:n][rng.permutation(n)]
    bu, bv = m.copy(), np.full(n, R, dtype=np.int64)
    kind = np.arange(n) % 7
    bv[kind == 1] = bu[kind == 1]                                        # self-loops, seen and fresh
    bv[kind == 3] = st.root[bu[kind == 3]]                               # already joined (or a self-loop)
    if st.u.size:
        j = np.nonzero(kind == 5)[0]
        bu[j], bv[j] = st.u[j % st.u.size], st.v[j % st.u.size]          # edges of the pre-state again
    far = [CAP, CAP + 3, 0x7FFFFFFF] if bits == 32 else [CAP, -3, 2 ** 32 + 5, 2 ** 40]
    j = np.nonzero(kind == 6)[0]
    bad_u = bu.copy()
    bad_v = bv.copy()
    bad_u[j[0::2]] = np.resize(far, j[0::2].size)                        # u out of range, then v
    bad_v[j[1::2]] = np.resize(far, j[1::2].size)
    keep = np.ones(n, bool)
    keep[j] = False
    want = _oracle(oracle, st, bu[keep], bv[keep])
    dt = np.int32 if bits == 32 else np.int64
    for how in ("fold_pairs", "fold"):
        st.enter(torch, ds)
        if how == "fold_pairs":
            ds.fold_pairs(torch.from_numpy(_interleave(bad_u, bad_v, dt)).cuda())
        else:
            ds.fold(torch.from_numpy(bad_u.astype(dt)).cuda(), torch.from_numpy(bad_v.astype(dt)).cuda())
        with pytest.raises(GsError) as ei:
            ds.sync()
        assert ei.value.code == _abi.GS_ERR_RANGE, how
        assert _equal(ds, want), how


@pytest.mark.parametrize("bits", [32, 64])
def test_four_pairs_per_thread(oracle, torch_cuda, handles, bits):
    """2^22 + 1024 + 3 pairs over 2^20 ids into a mature summary: the 1024-pair head launch
    (kMergeHead) and a remainder above kSmallPairFold (k_fold<..., AOS, ..., EPT 4>) with a ragged
    tail. 64 shared roots; 2^19 members in distinct components (path tails, middles, roots, untouched
    ids), always with the same root, in runs of 256 pairs on one root, so every lane of a wave
    shares H. The first 2^18 members come once, at the head of the batch, the others about 15 times: a
    root is the larger one only until its first hook, so only the first pairs to arrive combine,
    and a repeated pair would put back a union that a combined hook had lost."""
    torch = torch_cuda
    cap = 1 << 20
    st = PreState.__new__(PreState)
    st.name, st.cap, st._dev = "paths", cap, {}
    st.u, st.v = _paths3(0, cap // 8)
    n = (1 << 22) + 1024 + 3
    nm = 1 << 19
    k = np.arange(cap // 8, dtype=np.int64)
    members = np.concatenate([3 * k + np.array([2, 0, 1])[k % 3], 3 * (cap // 8) + np.arange(nm - cap // 8)])
    assert members.size == nm and members.max() < cap - FAMILIES
    members = members[np.random.default_rng(5).permutation(nm)]
    i = np.arange(n, dtype=np.int64)
    i = np.where(i < nm, i, nm // 2 + (i - nm) % (nm // 2))
    bu, bv = members[i], (cap - 1) - (i // 256) % FAMILIES
    ds = handles(bits, cap)
    st.enter(torch, ds)
    dt = np.int32 if bits == 32 else np.int64
    ds.fold_pairs(torch.from_numpy(_interleave(bu, bv, dt)).cuda())
    assert _equal(ds, _oracle(oracle, st, bu, bv))
    ds.reset()


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("state", ["s0", "s1"])
def test_marks_under_combined_hooks(oracle, torch_cuda, states, state, bits):
    """C: a family-A batch (n = 129) and a family-B batch (n = 513) folded into a marking handle A;
    its export folded into a fresh handle B carries all of it. The export holds one pair per vertex
    whose root status changed (include/gsgpu.h, gs_cc_export_marks: the roots this handle hooked —
    every vertex is hooked at most once): the vertices that were a root or untouched before the
    batches and hang below another vertex after them. A rewritten union(lo, Lmin) must have marked
    lo, the root it really hooked, not R."""
    torch = torch_cuda
    st = states[state]
    dt = np.int32 if bits == 32 else np.int64
    a = DisjointSet(CAP, id_bits=bits, track_marks=True)
    b = DisjointSet(CAP, id_bits=bits)
    buf = torch.empty(4 * CAP, dtype=torch.int32, device="cuda")
    st.enter(torch, a)
    m0 = a.export_marks(buf)                                   # the pre-state's own hooks
    b.fold_pairs(buf, m0, id_bits=32)
    b.sync()                                                   # buf is written again below
    rng = np.random.default_rng(17)
    au, av = st.pool[True][:129][rng.permutation(129)], np.full(129, R)
    bu = st.pool[False][200:713][rng.permutation(513)]         # other members, five other roots
    bv = (R - 1) - np.arange(513) % 5
    us, vs = np.concatenate([au, bu]), np.concatenate([av, bv])
    a.fold_pairs(torch.from_numpy(_interleave(au, av, dt)).cuda())
    a.fold_pairs(torch.from_numpy(_interleave(bu, bv, dt)).cuda())
    m = a.export_marks(buf)
    pairs = buf[:2 * m].view(-1, 2).cpu().numpy().astype(np.int64)
    b.fold_pairs(buf, m, id_bits=32)
    want = _oracle(oracle, st, us, vs)
    fin = want["final"]
    was_root = (st.labels < 0) | (st.labels == np.arange(CAP))
    hooked = np.nonzero(was_root & (fin >= 0) & (fin != np.arange(CAP)))[0]
    assert m == hooked.size
    assert sorted(pairs[:, 0].tolist()) == hooked.tolist()
    assert _equal(a, want)
    assert _equal(b, want)
    a.close()
    b.close()


def _star_window(world, k, seed):
    """Two windows of world * k edges. The second is the directed one: rank 0's slice (v_i, s_i),
    distinct s_i < 1000; rank r's the star (v_i, c_r) on a centre c_r = 1000 + r below every v_i,
    which rank 0 never touches — so every pair rank r exports names the root c_r, the larger root
    of each union on the receiver. The first window (rank r: the self-loop on 3900 + r, k times)
    only sizes the speculative slots: the first window of a stream is an exact round
    (exchange_plan.hpp exact_round, comm.hip exchange_exact), which folds through
    gs_cc_fold_pairs' kernel; the slot folds run from the second window on."""
    rng = np.random.default_rng(seed)
    v = 2000 + rng.permutation(1500)[:k].astype(np.int64)
    first = np.repeat(3900 + np.arange(world, dtype=np.int64), k)
    s = [first] + [v] * world
    d = [first, rng.permutation(1000)[:k].astype(np.int64)] + [np.full(k, 1000 + r, dtype=np.int64) for r in range(1, world)]
    return np.concatenate(s), np.concatenate(d)


@pytest.mark.parametrize("mode", ["allgather", "gather"])
@pytest.mark.parametrize("world", [2, 3])
def test_slot_folds_of_one_sender_root(oracle, world, mode):
    """D: k_fold_slots through the all-gather and gather exchanges, slices of 3, 65, 129 and 257
    pairs per rank in the directed window (_star_window)."""
    for k in (3, 65, 129, 257):
        s, d = _star_window(world, k, 50 + k)
        W = s.size // 2
        want = oracle.run(s, d, W, partitions=world, emit=EMIT_CHECKSUM, label_cap=CAP, want_final=True)
        sums, finals, _ = _run_local(world, mode, s, d, CAP, W)
        assert len(sums[0]) == 2
        for r in (range(world) if mode == "allgather" else [0]):
            assert sums[r] == [int(x) for x in want["checksums"]], "k %d rank %d" % (k, r)
            np.testing.assert_array_equal(finals[r], want["final"], err_msg="k %d rank %d" % (k, r))


def _slot_ordered_long_ids(cap):
    """ids[x], x < cap: Java longs (from _long_ids) whose slots are ordered like x. A sparse summary
    unions slot numbers, slot = splitmix64(id) >> (64 - hbits) with 2^hbits = 2 x capacity
    (sparse_ids.hpp sparse_home; no probing while the homes in use are distinct), so which root of a
    union is the larger one follows the slots, not the ids."""
    hbits = max(4, (2 * cap - 1).bit_length())
    cand = _long_ids(np.arange(4 * cap))
    home = _np_splitmix64(cand.view(np.uint64)) >> np.uint64(64 - hbits)
    _, first = np.unique(home, return_index=True)            # one id per home, homes ascending
    assert first.size >= cap
    return cand[first[:cap]]


@pytest.mark.parametrize("mode", ["allgather", "gather"])
def test_slot_folds_of_one_sender_root_sparse_ids(oracle, mode):
    """The same through k_fold_slots_sparse: arbitrary Java longs, (id, root id) int64 pairs, the
    ids chosen so that their slots keep the order of the dense case."""
    ids = _slot_ordered_long_ids(CAP)
    for k in (3, 65, 129, 257):
        s, d = _star_window(2, k, 80 + k)
        s, d = ids[s], ids[d]
        W = s.size // 2
        want = oracle.run(s, d, W, partitions=2, emit=EMIT_CHECKSUM, label_cap=0)
        sums, _, _ = _run_local(2, mode, s, d, CAP, W, sparse=True)
        assert len(sums[0]) == 2
        for r in (range(2) if mode == "allgather" else [0]):
            assert sums[r] == [int(x) for x in want["checksums"]], "k %d rank %d" % (k, r)
