"""Neighbourhood slices (gs_slice_reduce_windows) on an RMAT stream with edge values: scale 20, edge
factor 16, seed 1 (gsgpu.gen.rmat), values a seeded 64-bit mix of the edge index, 2^20-edge windows,
every window of the stream through ONE call per step. Cases: SUM under "out" and under "all".
Prints one JSON line: edges/s and ms per step (medians over --steps), rows per window and the
longest row, and with --cpu-baseline the time of the numpy restatement (tests/slices_oracle.py,
oracle (b)) of the same windows on the host's cores, whose records must equal the device's.

The step time is a host clock around the call, which ends in its one host wait. Edges and values are
generated on the device before the clock starts and the records stay on the device; ids are 32 bits
wide unless --id-bits 64.

--ab LIB alternates this library with another build of it (an experiment library of `make exp`,
e.g. gsgpu/lib/exp/libgsgpu_SLICE_PAYLOAD.so, which carries the values through the sort instead of
gathering them through the sorted positions): --pairs times, one fresh process per run, A B A B ...;
the line then holds every run's medians side by side.
usage: python tools/bench_slices.py [--steps K] [--warmup W] [--cases out,all] [--cpu-baseline] [--ab LIB --pairs 3]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gelly-streaming_amd"))
C1, C2 = -7046029254386353131, -4658895280553007687          # 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9 as int64


def edge_values(torch, n, seed):
    """A 64-bit mix of the edge index (wrapping int64 arithmetic; >> is the arithmetic shift)."""
    x = (torch.arange(n, device="cuda", dtype=torch.int64) + seed) * C1
    x = (x ^ (x >> 32)) * C2
    return (x ^ (x >> 29)).contiguous()


def run(args):
    import numpy as np
    import torch
    import gsgpu
    from gsgpu import _abi, gen

    if not torch.cuda.is_available():
        raise SystemExit("bench_slices.py needs a HIP device; there is no CPU path to time")
    torch.cuda.set_device(0)
    dt = torch.int32 if args.id_bits == 32 else torch.int64
    nv, n, W = 1 << args.scale, args.edge_factor << args.scale, args.window_edges
    src = torch.empty(n, dtype=dt, device="cuda")
    dst = torch.empty(n, dtype=dt, device="cuda")
    gen.rmat(src, dst, 0, args.scale, args.seed)
    val = edge_values(torch, n, args.seed)
    torch.cuda.synchronize()
    out = {"what": "gs_slice_reduce_windows SUM, RMAT scale %d edge factor %d seed %d with 64-bit values, %d-edge windows, "
                   "one call per step" % (args.scale, args.edge_factor, args.seed, W),
           "id_bits": args.id_bits, "steps": args.steps, "warmup": args.warmup, "edges": n, "windows": -(-n // W),
           "device": torch.cuda.get_device_name(0), "lib": os.path.basename(_abi.LIB_PATH),
           "lib_source_sha": _abi.lib_source_sha(), "cases": {}}
    for d in args.cases.split(","):
        entries = 2 * n if d == "all" else n
        ov = torch.empty(entries, dtype=dt, device="cuda")
        ox = torch.empty(entries, dtype=torch.int64, device="cuda")
        times, first = [], None
        with gsgpu.SnapshotStream(nv, d, id_bits=args.id_bits) as ss:
            for step in range(args.warmup + args.steps):
                ss.sync()
                t0 = time.perf_counter()
                offs, st = ss.reduce_windows(src, dst, val, W, "sum", out=(ov, ox))
                t = time.perf_counter() - t0
                if step >= args.warmup:
                    times.append(t)
                if first is not None and (offs.tolist(), st.tolist()) != first:
                    raise SystemExit("%s: offsets or statistics changed between steps" % d)
                first = (offs.tolist(), st.tolist())
        ts = sorted(times)
        med = ts[len(ts) // 2]
        row = {"entries": entries, "ms_per_step": med * 1e3, "ms_per_step_min": ts[0] * 1e3, "ms_per_step_max": ts[-1] * 1e3,
               "edges_per_s": n / med, "entries_per_s": entries / med,
               "rows_per_window": [int(x) for x in st["n_vertices"]], "longest_row": [int(x) for x in st["max_row"]],
               "checksum_xor": "%016x" % int(np.bitwise_xor.reduce(st["checksum"]))}
        if args.cpu_baseline:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import slices_oracle
            hs, hd, hx = src.cpu().numpy().astype(np.int64), dst.cpu().numpy().astype(np.int64), val.cpu().numpy()
            gv, gx = ov.cpu().numpy().astype(np.int64), ox.cpu().numpy()
            cpu = 0.0
            for k in range(len(offs) - 1):
                w = slice(k * W, min(k * W + W, n))
                t0 = time.perf_counter()
                cv, cx = slices_oracle.numpy_reduce(hs[w], hd[w], hx[w], d, "sum")
                cpu += time.perf_counter() - t0
                a, b = int(offs[k]), int(offs[k + 1])
                if not (np.array_equal(cv, gv[a:b]) and np.array_equal(cx, gx[a:b])):
                    raise SystemExit("%s window %d: the numpy restatement disagrees with the device" % (d, k))
                if slices_oracle.checksum_arrays(cv, cx) != int(st["checksum"][k]):
                    raise SystemExit("%s window %d: checksum mismatch" % (d, k))
            row["cpu_numpy_s_per_step"] = cpu
            row["cpu_numpy_edges_per_s"] = n / cpu
            row["cpu_equals_device"] = True
        out["cases"][d] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edge-factor", type=int, default=16)
    ap.add_argument("--window-edges", type=int, default=1 << 20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--id-bits", type=int, default=32, choices=(32, 64))
    ap.add_argument("--cases", default="out,all")
    ap.add_argument("--cpu-baseline", action="store_true")
    ap.add_argument("--ab", default=None, help="another build of the library to alternate with")
    ap.add_argument("--pairs", type=int, default=3)
    args = ap.parse_args()
    if not args.ab:
        print(json.dumps(run(args)))
        return
    # one fresh process per run (the library is chosen when it is loaded); this process opens no device
    base = [sys.executable, os.path.abspath(__file__)] + [a for a in sys.argv[1:]]
    cut = base.index("--ab")
    del base[cut:cut + 2]
    runs = []
    for pair in range(args.pairs):
        for name, lib in (("product", None), ("other", os.path.abspath(args.ab))):
            env = dict(os.environ)
            env.pop("GSGPU_LIB", None)
            if lib:
                env["GSGPU_LIB"] = lib
            line = subprocess.check_output(base, env=env, timeout=900).decode().strip().splitlines()[-1]
            r = json.loads(line)
            runs.append({"pair": pair, "which": name, "lib": r["lib"],
                         "ms_per_step": {d: c["ms_per_step"] for d, c in r["cases"].items()},
                         "checksum_xor": {d: c["checksum_xor"] for d, c in r["cases"].items()}})
    if len({json.dumps(r["checksum_xor"], sort_keys=True) for r in runs}) != 1:
        raise SystemExit("the two builds disagree on the checksums")
    print(json.dumps({"what": "bench_slices.py --ab: the product library and %s alternated, %d pairs" % (os.path.basename(args.ab), args.pairs),
                      "runs": runs}))


if __name__ == "__main__":
    main()
