"""The ring fold's round scheduler against the C oracle (run as a SUBPROCESS of
tests/test_gpu_ring_steal.py: the library reads GSGPU_RING_STEAL, GSGPU_RING_MIN_BITS,
GSGPU_FOLD_MODE and GSGPU_FOLD_STATS once per process; csrc/cc_api.hip).

k_fold_ring (csrc/cc_kernels.hpp, RingSteal) runs all but the last rows of a workgroup's grid-stride
rounds statically and hands the wave rounds of the last rows out through per-workgroup counters, to
the owner's waves and to those of a few other workgroups; the counters live in two sets that
alternate between launches, each launch zeroing the other set. Two streams, ids below 2^21:

  sequence  windows of alternating sizes (large, tiny, large, small, ...), one ring launch each once
            the forest is mature: 2^22 edges (4 rows per workgroup at G = 256: all of them tickets
            with the production tail of 4 rows, 2 static rows and 2 rows of tickets with
            GSGPU_RING_STEAL=2), 2^23 edges (8 rows: 4 static, then 4 of tickets, the shape of
            the headline's 12 + 4), 4, 252, 256 and
            260 edges (one workgroup, a partial wave, one or two wave rounds), 4*1024*3 + 4 (the
            last workgroup owns one group), 4*1024*G*2 + 4*64*5 + 4 with G the CU count (a ragged
            last row with fewer wave rounds than workgroups). A counter set that was not zeroed, or
            zeroed only up to a smaller launch's grid, hands out too few rounds in a later window.
  forced    windows of 2^22 edges in which the rounds owned by 8 of the G workgroups (positions p
            with (p / 4096) % G < 8) hold only first touches next to the giant, every one a union,
            and all other positions edges inside the giant: the other workgroups drain their rounds
            long before those 8, whose tails are then expected to be stolen (with GSGPU_RING_STEAL=2
            from behind 2 static rows). Nothing observes a steal (no test may depend on timing):
            what is checked is that every edge is folded exactly once whoever runs its round.

--make-ref PATH  writes both streams and the oracle's per-window checksums and final labels.
--ref PATH       folds them window by window on a plain and on a track_marks handle, with int32
                 and int64 ids, and compares every window; prints one JSON line. `stats_valid` is
                 the `valid` count GSGPU_FOLD_STATS must report for every close, in order.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "gelly-streaming_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

CAP = 1 << 21
BIG = 1 << 22
BIG2 = 1 << 23


def sequence_sizes(G: int):
    ragged = 4 * 1024 * G * 2 + 4 * 64 * 5 + 4
    last_one = 4 * 1024 * 3 + 4
    return [BIG, 4, ragged, 252, BIG2, 256, ragged, 260, last_one]


def sequence_stream(G: int):
    """Skewed ids (a few hubs, a long tail) below 2^21: a giant forms in window 0 and the hot and warm
    sets fill, as on an RMAT stream."""
    sizes = sequence_sizes(G)
    rng = np.random.default_rng(9)
    n = int(sum(sizes))
    s = (rng.random(n) ** 3 * CAP).astype(np.int64)
    d = (rng.random(n) ** 3 * CAP).astype(np.int64)
    return s, d, sizes


def forced_stream(G: int, windows: int = 2, seed: int = 5):
    """Window 0 (2^21 edges) joins [0, 2^20) into one component (a path plus random edges,
    shuffled); windows 1.. (2^22 edges): position p of the window is owned by workgroup (p / 4096) % G of its
    ring launch."""
    rng = np.random.default_rng(seed)
    half, W0, W = CAP // 2, BIG // 2, BIG
    s0 = np.concatenate([np.arange(half - 1), rng.integers(0, half, W0 - (half - 1))])
    d0 = np.concatenate([np.arange(1, half), rng.integers(0, half, W0 - (half - 1))])
    perm = rng.permutation(W0)
    src, dst = [s0[perm]], [d0[perm]]
    fresh = half
    slow = ((np.arange(W) // 4096) % G) < 8
    for _ in range(windows):
        s = rng.integers(0, half, W)
        d = rng.integers(0, half, W)
        k = int(slow.sum())
        assert fresh + k <= CAP
        new = np.arange(fresh, fresh + k)
        fresh += k
        flip = rng.integers(0, 2, k).astype(bool)           # the fresh vertex on either side
        a, b = s[slow].copy(), new.copy()
        a[flip], b[flip] = new[flip], s[slow][flip]
        s[slow], d[slow] = a, b
        src.append(s)
        dst.append(d)
    return np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64), [W0] + [W] * windows


def oracle_windows(oracle, s, d, sizes):
    """Checksum after every window of the given sizes and the final dense labels: the oracle run
    window by window, each run restored from the labels the one before ended with."""
    from pyoracle import EMIT_CHECKSUM
    sums, init, lo, final = [], None, 0, None
    for n in sizes:
        r = oracle.run(s[lo:lo + n], d[lo:lo + n], 0, partitions=1, threads=1, emit=EMIT_CHECKSUM, label_cap=CAP,
                       want_final=True, init=init)
        final = r["final"]
        seen = np.nonzero(final >= 0)[0]
        init = (seen, final[seen])
        sums.append(int(r["checksums"][-1]))
        lo += n
    return np.array(sums, dtype=np.uint64), final


def make_ref(path: str, G: int):
    from pyoracle import coracle
    oracle = coracle()
    s, d, sizes = sequence_stream(G)
    sums, final = oracle_windows(oracle, s, d, sizes)
    fs, fd, fsizes = forced_stream(G)
    fsums, ffinal = oracle_windows(oracle, fs, fd, fsizes)
    np.savez(path, G=G, seq_s=s.astype(np.int32), seq_d=d.astype(np.int32), seq_sizes=np.array(sizes), seq_sums=sums,
             seq_final=final, forced_s=fs.astype(np.int32), forced_d=fd.astype(np.int32),
             forced_sizes=np.array(fsizes), forced_sums=fsums, forced_final=ffinal)


def run_case(torch, name, s, d, sizes, sums, final, id_bits, track_marks):
    import gsgpu
    dt = torch.int32 if id_bits == 32 else torch.int64
    ts = torch.from_numpy(s).cuda().to(dt)
    td = torch.from_numpy(d).cuda().to(dt)
    ds = gsgpu.DisjointSet(CAP, id_bits=id_bits, track_marks=track_marks, stream=torch.cuda.current_stream())
    bad, lo = None, 0
    for w, n in enumerate(sizes):
        n = int(n)
        ds.fold(ts[lo:lo + n], td[lo:lo + n])
        ds.close_window()
        if ds.checksum()[0] != int(sums[w]) and bad is None:
            bad = w
        lo += n
    final_ok = bool(np.array_equal(ds.dense().astype(np.int64), final))
    ds.close()
    return {"case": "%s/int%d/%s" % (name, id_bits, "marks" if track_marks else "plain"), "windows": len(sizes),
            "first_bad_window": bad, "final_equal": final_ok, "ok": bad is None and final_ok}


def check(path: str):
    import torch
    assert torch.cuda.is_available()
    z = np.load(path)
    G = torch.cuda.get_device_properties(0).multi_processor_count
    assert int(z["G"]) == G, "the reference was made for another CU count"
    res, stats_valid = [], []
    for name in ("seq", "forced"):
        for id_bits in (32, 64):
            for marks in (False, True):
                sizes = [int(x) for x in z[name + "_sizes"]]
                res.append(run_case(torch, name, z[name + "_s"], z[name + "_d"], sizes, z[name + "_sums"],
                                    z[name + "_final"], id_bits, marks))
                stats_valid += sizes
    env = {k: v for k, v in os.environ.items() if k.startswith("GSGPU_")}
    print(json.dumps({"env": env, "ok": all(r["ok"] for r in res), "cases": res, "stats_valid": stats_valid}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make-ref", default=None, metavar="PATH")
    ap.add_argument("--ref", default=None, metavar="PATH")
    ap.add_argument("--cus", type=int, default=0, help="with --make-ref: the CU count (default: ask the device)")
    a = ap.parse_args()
    if a.make_ref:
        G = a.cus
        if not G:
            import torch
            G = torch.cuda.get_device_properties(0).multi_processor_count
        make_ref(a.make_ref, G)
    if a.ref:
        check(a.ref)


if __name__ == "__main__":
    main()
