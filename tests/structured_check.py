"""Structured streams through one fold configuration against the C oracle (run as a SUBPROCESS of
tests/test_gpu_structured_ring.py: the library reads GSGPU_FOLD_MODE and GSGPU_RING_MIN_BITS once
per process; csrc/cc_api.hip).

tests/structured_streams.py's comb, equal_paths, star_max_hub and desc_path at the capacity
2^20 + 3 (21 id bits: the ring fold and its warm set with GSGPU_RING_MIN_BITS=20): k_fold_ring's
giant filter, hot-set and warm-set admission and claims against a giant that is a comb, a star
whose root is renamed by every smaller leaf, or a chain re-rooted by every edge, and many mature
windows with no giant at all.

--make-ref PATH  writes the streams and the oracle's per-window checksums and final labels.
--ref PATH       folds each stream window by window (fold + close_window) and through
                 fold_windows (one call, then calls of 3 windows), int32 device arrays, every window
                 compared; prints one JSON line. With GSGPU_FOLD_MODE=ring or GSGPU_RING_MIN_BITS
                 set, the window-by-window handle times GS_K_RING launches (gs_cc_timing) and the
                 line reports their number per case (`ring_launches`); a `comb` run without a ring
                 launch is not ok: a run that never reached k_fold_ring must not pass.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "gelly-streaming_amd"), os.path.join(ROOT, "oracle"), HERE):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import structured_streams as ss  # noqa: E402

CASES = ("comb", "equal_paths", "star_max_hub", "desc_path")


def make_ref(path: str):
    from pyoracle import coracle
    oracle = coracle()
    out = {}
    for name in CASES:
        s, d = ss.stream(name)
        want = ss.oracle_windows(oracle, name)
        out[name + "_s"] = s.astype(np.int32)
        out[name + "_d"] = d.astype(np.int32)
        out[name + "_sums"] = want["checksums"]
        out[name + "_final"] = want["final"]
    np.savez(path, **out)


def ring_expected() -> bool:
    return os.environ.get("GSGPU_FOLD_MODE") == "ring" or bool(os.environ.get("GSGPU_RING_MIN_BITS"))


def run_case(torch, name, s, d, sums, final, ring):
    import gsgpu
    from gsgpu import _abi
    N, W = ss.N, ss.W
    ts = torch.from_numpy(s).cuda()
    td = torch.from_numpy(d).cuda()
    nwin = len(sums)
    ds = gsgpu.DisjointSet(N, id_bits=32, stream=torch.cuda.current_stream())
    if ring:
        ds.timing(_abi.GS_TIMING_MASK | (1 << _abi.GS_K_RING))
    bad = None
    for w in range(nwin):
        ds.fold(ts[w * W:(w + 1) * W], td[w * W:(w + 1) * W])
        ds.close_window()
        if ds.checksum()[0] != int(sums[w]) and bad is None:
            bad = w
    final_ok = bool(np.array_equal(ds.dense().astype(np.int64), final))
    launches = ds.kernel_time(_abi.GS_K_RING)[1] if ring else None
    ds.close()
    # fold_windows: the whole stream in one call, then calls of 3 windows
    ds = gsgpu.DisjointSet(N, id_bits=32, stream=torch.cuda.current_stream())
    fw_bad = None
    assert ds.fold_windows(ts, td, W) == nwin
    if ds.checksum()[0] != int(sums[-1]) or not np.array_equal(ds.dense().astype(np.int64), final):
        fw_bad = nwin - 1
    ds.reset()
    for w0 in range(0, nwin, 3):
        k = min(3, nwin - w0)
        assert ds.fold_windows(ts[w0 * W:(w0 + k) * W], td[w0 * W:(w0 + k) * W], W) == k
        if ds.checksum()[0] != int(sums[w0 + k - 1]) and fw_bad is None:
            fw_bad = w0 + k - 1
    fw_final_ok = bool(np.array_equal(ds.dense().astype(np.int64), final))
    ds.close()
    ok = bad is None and final_ok and fw_bad is None and fw_final_ok
    if ring and name == "comb":
        ok = ok and launches >= 1
    return {"case": name, "windows": nwin, "first_bad_window": bad, "final_equal": final_ok,
            "fold_windows_first_bad": fw_bad, "fold_windows_final_equal": fw_final_ok, "ring_launches": launches,
            "ok": bool(ok)}


def check(path: str):
    import torch
    assert torch.cuda.is_available()
    z = np.load(path)
    ring = ring_expected()
    res = [run_case(torch, name, z[name + "_s"], z[name + "_d"], z[name + "_sums"], z[name + "_final"], ring)
           for name in CASES]
    env = {k: v for k, v in os.environ.items() if k.startswith("GSGPU_")}
    print(json.dumps({"env": env, "ring_expected": ring, "ok": all(r["ok"] for r in res), "cases": res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make-ref", default=None, metavar="PATH")
    ap.add_argument("--ref", default=None, metavar="PATH")
    a = ap.parse_args()
    if a.make_ref:
        make_ref(a.make_ref)
    if a.ref:
        check(a.ref)


if __name__ == "__main__":
    main()
