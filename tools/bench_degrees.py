"""Streaming degrees (gs_deg_fold_windows) on RMAT event streams: scale 20 and 24, edge factor 16,
seed 1 (gsgpu.gen.rmat), 2^20-event windows, one call per step. Three streams per scale:
  add        all additions (add == NULL: one host wait per call)
  del_prior  every tenth event from the second window on deletes an edge added one window earlier
             (each such edge once), so no vertex is ever at risk
  del_random every tenth event deletes a random pair, so some vertices are at risk (and clamp)
For each stream the counting path (GS_DEG_COUNT) and sort-everything (GS_DEG_SORT_ALL, the default) are timed alternately, step by step,
on the same device in the same process. Prints one JSON line: events/s, ms per step, the share of
windows and of vertex events that took the exact path, and with --cpu-baseline the time of a numpy
restatement (bincount) of the first window of the all-additions stream.

The step time is a host clock around reset + the call, which ends in its host wait. Events are
generated on the device before the clock starts; ids are 32 bits wide unless --id-bits 64.
usage: python tools/bench_degrees.py [--scales 20,24] [--steps K] [--warmup W] [--cpu-baseline] [--only count|sort_all]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gelly-streaming_amd"))


def make_streams(torch, gen, scale, n, W, seed, dt):
    src = torch.empty(n, dtype=dt, device="cuda")
    dst = torch.empty(n, dtype=dt, device="cuda")
    gen.rmat(src, dst, 0, scale, seed)
    torch.cuda.synchronize()
    idx = torch.arange(n, device="cuda")
    dele = (idx % 10 == 9) & (idx >= W)
    where = idx[dele]
    del idx
    add = (~dele).to(torch.uint8).contiguous()
    # W - 1 back: (9 - W % 10 - 1) % 10 != 9 for W = 2^20 (W % 10 == 6), so the target is an addition
    assert (9 - W % 10 - 1) % 10 != 9
    s1, d1 = src.clone(), dst.clone()
    s1[where] = src[where - W - 1]
    d1[where] = dst[where - W - 1]
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    s2, d2 = src.clone(), dst.clone()
    s2[where] = torch.randint(0, 1 << scale, (where.numel(),), device="cuda", generator=g).to(dt)
    d2[where] = torch.randint(0, 1 << scale, (where.numel(),), device="cuda", generator=g).to(dt)
    torch.cuda.synchronize()
    return {"add": (src, dst, None), "del_prior": (s1, d1, add), "del_random": (s2, d2, add)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scales", default="20,24")
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--window-edges", type=int, default=1 << 20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--id-bits", type=int, default=32, choices=(32, 64))
    ap.add_argument("--only", default=None, choices=("count", "sort_all"))
    ap.add_argument("--cpu-baseline", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch
    import gsgpu
    from gsgpu import _abi, gen

    if not torch.cuda.is_available():
        raise SystemExit("bench_degrees.py needs a HIP device; there is no CPU path to time")
    torch.cuda.set_device(0)
    dt = torch.int32 if args.id_bits == 32 else torch.int64
    W = args.window_edges
    paths = [p for p in ("count", "sort_all") if args.only in (None, p)]
    out = {"what": "gs_deg_fold_windows, RMAT edge factor %d seed %d, %d-event windows, one call per step; "
                   "counting path (GS_DEG_COUNT) and GS_DEG_SORT_ALL (= default flags) alternated step by step" % (args.edge_factor, args.seed, W),
           "id_bits": args.id_bits, "steps": args.steps, "warmup": args.warmup, "streams": {},
           "device": torch.cuda.get_device_name(0), "lib_source_sha": _abi.lib_source_sha()}
    for scale in [int(x) for x in args.scales.split(",")]:
        nv, n = 1 << scale, args.edge_factor << scale
        streams = make_streams(torch, gen, scale, n, W, args.seed, dt)
        for name, (s, d, a) in streams.items():
            hs = {p: gsgpu.DegreeSummary(nv, id_bits=args.id_bits, path=("sort" if p == "sort_all" else "count")) for p in paths}
            times = {p: [] for p in paths}
            stats = {}
            for step in range(args.warmup + args.steps):
                for p in paths:                             # alternated on the same box
                    h = hs[p]
                    h.sync()
                    t0 = time.perf_counter()
                    h.reset()
                    st = h.fold_windows(s, d, W, a)
                    t = time.perf_counter() - t0
                    if step >= args.warmup:
                        times[p].append(t)
                    if p in stats and st.tolist() != stats[p].tolist():
                        raise SystemExit("%s/%s: statistics changed between steps" % (name, p))
                    stats[p] = st
            if len(paths) == 2 and stats["count"].tolist() != stats["sort_all"].tolist():
                raise SystemExit("%s scale %d: the two paths disagree" % (name, scale))
            row = {"events": n, "vertex_events": 2 * n, "windows": int(stats[paths[0]].size),
                   "final": {k: int(stats[paths[0]][-1][k]) for k in stats[paths[0]].dtype.names}}
            for p in paths:
                ts = sorted(times[p])
                med = ts[len(ts) // 2]
                pc = hs[p].path_counts()
                row[p] = {"ms_per_step": med * 1e3, "ms_per_step_min": ts[0] * 1e3, "ms_per_step_max": ts[-1] * 1e3,
                          "events_per_s": n / med,
                          "exact_window_share": pc["exact_windows"] / max(pc["windows"], 1),
                          "exact_vertex_event_share": pc["exact_events"] / max(pc["vertex_events"], 1)}
                hs[p].close()
            if args.cpu_baseline and name == "add":
                hsrc, hdst = s[:W].cpu().numpy(), d[:W].cpu().numpy()
                t0 = time.perf_counter()
                deg = np.bincount(hsrc, minlength=nv) + np.bincount(hdst, minlength=nv)
                dist = np.bincount(deg[deg > 0])
                row["cpu_numpy_window0_s"] = time.perf_counter() - t0
                st0 = stats[paths[0]][0]
                if (int(np.count_nonzero(deg)), int(np.count_nonzero(dist)), int(deg.max())) != \
                        (int(st0["n_vertices"]), int(st0["n_degrees"]), int(st0["max_degree"])):
                    raise SystemExit("the numpy restatement of window 0 disagrees with the device")
            out["streams"]["scale%d_%s" % (scale, name)] = row
        del streams
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
