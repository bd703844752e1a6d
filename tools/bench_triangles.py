"""Per-window triangle counts (gs_tri_count_windows) on an RMAT stream: scale 20, edge factor 16,
seed 1 (gsgpu.gen.rmat), counted in 2^20-edge windows by one call per step. Prints one JSON line:
edges/s, ms per step, the triangles of every window and, with --cpu-baseline, the time a numpy
restatement (degree-oriented sorted rows, one window) takes on the first window.

The step time is a host clock around the call, which ends in its one host wait. Edges are
generated on the device before the clock starts; ids are 32 bits wide unless --id-bits 64.
usage: python tools/bench_triangles.py [--steps K] [--warmup W] [--orient degree|id] [--cpu-baseline]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gelly-streaming_amd"))


def cpu_window_count(src, dst, nv, chunk=1 << 16):
    """Triangles of one window with numpy: distinct edges directed low (degree, id) -> high,
    every wedge a -> b, a -> w looked up as the edge b -> w among the sorted edges."""
    import numpy as np
    src, dst = src.astype(np.int64), dst.astype(np.int64)
    keep = src != dst
    lo, hi = np.minimum(src, dst)[keep], np.maximum(src, dst)[keep]
    key = np.unique(lo * nv + hi)
    lo, hi = key // nv, key % nv
    deg = np.bincount(lo, minlength=nv) + np.bincount(hi, minlength=nv)
    flip = deg[lo] > deg[hi]
    a, b = np.where(flip, hi, lo), np.where(flip, lo, hi)
    key = np.sort(a * nv + b)
    a, b = key // nv, key % nv
    start = np.searchsorted(a, np.arange(nv), side="left")
    out = np.bincount(a, minlength=nv)
    total = 0
    for c0 in range(0, a.size, chunk):
        ea = a[c0:c0 + chunk]
        reps = out[ea]
        e = np.repeat(np.arange(ea.size), reps)
        within = np.arange(int(reps.sum())) - np.repeat(np.cumsum(reps) - reps, reps)
        w = b[start[ea[e]] + within]
        want = b[c0:c0 + chunk][e] * nv + w
        pos = np.minimum(np.searchsorted(key, want), key.size - 1)
        total += int((key[pos] == want).sum())
    return total, int(key.size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--window-edges", type=int, default=1 << 20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--id-bits", type=int, default=32, choices=(32, 64))
    ap.add_argument("--orient", default="degree", choices=("degree", "id"))
    ap.add_argument("--cpu-baseline", action="store_true")
    args = ap.parse_args()

    import torch
    import gsgpu
    from gsgpu import _abi, gen

    if not torch.cuda.is_available():
        raise SystemExit("bench_triangles.py needs a HIP device; there is no CPU path to time")
    torch.cuda.set_device(0)
    nv, n, W = 1 << args.scale, args.edge_factor << args.scale, args.window_edges
    dt = torch.int32 if args.id_bits == 32 else torch.int64
    src = torch.empty(n, dtype=dt, device="cuda")
    dst = torch.empty(n, dtype=dt, device="cuda")
    gen.rmat(src, dst, 0, args.scale, args.seed)
    torch.cuda.synchronize()

    tc = gsgpu.TriangleCounter(nv, id_bits=args.id_bits, orient=args.orient)
    counts = None
    for _ in range(args.warmup):
        counts = tc.count_windows(src, dst, W)
    times = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        got = tc.count_windows(src, dst, W)
        times.append(time.perf_counter() - t0)
        if counts is not None and got.tolist() != counts.tolist():
            raise SystemExit("counts changed between steps: %s vs %s" % (got.tolist(), counts.tolist()))
        counts = got
    simple0 = tc.simple_edges(src[:W], dst[:W])
    tc.close()
    times.sort()
    med = times[len(times) // 2]
    out = {"what": "gs_tri_count_windows, RMAT scale %d edge factor %d seed %d, %d-edge windows, one call per step"
                   % (args.scale, args.edge_factor, args.seed, W),
           "edges": n, "windows": int(counts.size), "id_bits": args.id_bits, "orient": args.orient,
           "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": med * 1e3, "ms_per_step_min": times[0] * 1e3, "ms_per_step_max": times[-1] * 1e3,
           "ms_per_window": med * 1e3 / max(int(counts.size), 1),
           "edges_per_s": n / med, "triangles_per_window": [int(c) for c in counts.tolist()],
           "simple_edges_window0": simple0,
           "device": torch.cuda.get_device_name(0), "lib_source_sha": _abi.lib_source_sha()}
    if args.cpu_baseline:
        hs, hd = src[:W].cpu().numpy(), dst[:W].cpu().numpy()
        t0 = time.perf_counter()
        total, m = cpu_window_count(hs, hd, nv)
        out["cpu_numpy_window0_s"] = time.perf_counter() - t0
        out["cpu_numpy_window0_triangles"] = total
        if total != int(counts[0]) or m != simple0:
            raise SystemExit("the numpy restatement counts %d triangles of %d edges, the device %d of %d"
                             % (total, m, int(counts[0]), simple0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
