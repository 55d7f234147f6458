#!/usr/bin/env python3
"""Time the RING <-> NEST reorder of full-sky maps on three routes, on one GPU.

    python tools/bench_reorder.py [--nside 1024] [--shapes 8x1,4x4,4x16,2x64] [--reps 50] [--warmup 5]

(kernel)       _native.healpix_reorder: dsph_healpix_reorder, no table (what HealpyReorder runs on a full-sky HIP map);
(rows_pack)    _native.rows_pack on a precomputed int32 table of 12 nside^2 entries: the library's route before that kernel;
(index_select) torch.index_select on the int64 table: what a user of the host framework writes.
Shapes are N x F (maps x channels), both directions each.  All routes run in this process, alternating, after a warm-up; times are
medians of device-event timings of single calls, with the smallest and largest beside them.  Bytes a reorder needs: the map in and
out, 2 N M F 4 (the tables' own bytes, 4 M and 8 M per call, are not counted); the rate is these bytes over the time, against the
6.3 TB/s an MI355X reaches from HBM.  Outputs are compared bit for bit before anything is timed.  Prints the figures and one JSON
line.  Needs a GPU: there is no CPU fallback and no figure without one.
"""

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deepsphere-cosmo-tf2_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from deepsphere import _native, healpix  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes / s


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nside", type=int, default=1024)
    ap.add_argument("--shapes", default="8x1,4x4,4x16,2x64", help="N x F, comma separated")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    _native.require_gpu()
    dev = torch.device("cuda", 0)
    nside, M = args.nside, 12 * args.nside * args.nside
    ids = np.arange(M, dtype=np.int64)
    # out[i] = in[table[i]]: to NEST through nest2ring, to RING through ring2nest
    t64 = {True: torch.as_tensor(healpix.nest2ring(nside, ids)).to(dev), False: torch.as_tensor(healpix.ring2nest(nside, ids)).to(dev)}
    t32 = {d: t.to(torch.int32) for d, t in t64.items()}
    results = []
    for N, F in shapes:
        x = torch.randn((N, M, F), generator=torch.Generator(device=dev).manual_seed(0), device=dev)
        outs = {name: torch.empty_like(x) for name in ("kernel", "rows_pack", "index_select")}
        alg = 2 * N * M * F * 4
        for to_nest in (True, False):
            cases = {
                "kernel": lambda: _native.healpix_reorder(x, nside, to_nest, out=outs["kernel"]),
                "rows_pack": lambda: _native.rows_pack(x, t32[to_nest], out=outs["rows_pack"]),
                "index_select": lambda: torch.index_select(x, 1, t64[to_nest], out=outs["index_select"]),
            }
            for fn in cases.values():  # same numbers first (faster and different is not faster)
                fn()
            torch.cuda.synchronize()
            same = all(torch.equal(outs["kernel"], outs[n]) for n in ("rows_pack", "index_select"))
            if not same:
                raise SystemExit(f"N {N} F {F} to_nest {to_nest}: the routes disagree")
            for _ in range(args.warmup):
                for fn in cases.values():
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name in cases}
            for _ in range(args.reps):  # alternating: drift of the machine hits every case alike
                for name, fn in cases.items():
                    times[name].append(timed(fn))
            ms = {name: statistics.median(t) for name, t in times.items()}
            direction = "ring->nest" if to_nest else "nest->ring"
            print(f"nside {nside}, N {N}, F {F}, {direction}: {alg / 1e9:.3f} GB in and out")
            for name in cases:
                rate = alg / (ms[name] * 1e-3)
                print(f"  {name:13s} {ms[name]:8.4f} ms  (min {min(times[name]):.4f}, max {max(times[name]):.4f}, {args.reps} calls)  "
                      f"{rate / 1e12:5.2f} TB/s = {rate / HBM_ACHIEVABLE:.2f} of {HBM_ACHIEVABLE / 1e12:.1f} TB/s", flush=True)
            results.append({"N": N, "F": F, "to_nest": to_nest, "bytes": alg, "ms": ms,
                            "min_ms": {n: min(t) for n, t in times.items()}, "max_ms": {n: max(t) for n, t in times.items()},
                            "hbm_fraction": {n: alg / (ms[n] * 1e-3) / HBM_ACHIEVABLE for n in ms}})
        del x, outs
    print(json.dumps({"nside": nside, "M": M, "reps": args.reps, "results": results}))


if __name__ == "__main__":
    main()
