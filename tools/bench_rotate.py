#!/usr/bin/env python3
"""Time the rotation of full-sky maps by HEALPix interpolation on four routes, on one GPU.

    python tools/bench_rotate.py [--nside 1024] [--shapes 8x1,4x4,4x16,2x64] [--reps 20] [--warmup 3] [--host-nside 256]

(kernel)       _native.healpix_rotate: dsph_healpix_rotate, nothing materialised (what HealpyRotate runs on a HIP map);
(ell_smooth)   _native.ell_smooth on the W = 4 table of _native.healpix_interp_table, built BEFOREHAND: one table and one launch for
               a shared rotation, a table and a launch per sample for per-sample rotations;
(torch)        four index_select and a weighted sum on the same table(s) (int64 columns), what a user of the host framework writes;
(host)         healpix.get_interp_val in numpy on the host plus the copy of the result to the device, at --host-nside: the
               hp.Rotator.rotate_map_pixel route (its stencil is computed per call, as healpy does).
Shapes are N x F (maps x channels), each with a fresh random rotation per sample and with one rotation for the batch.  The table
routes are timed on tables that exist; their build time (interp_table, one call per table) and memory (32 bytes per pixel and
rotation, 64 with the int64 columns of the torch route) are reported beside them and are NOT in their times -- a training loop that
draws a rotation per sample and step pays them every step.

All device routes run in this process, alternating, after a warm-up.  A RUN times --reps back-to-back calls of a route between two
device events; three runs per route, interleaved route by route; the figure is the median run, with the smallest and largest
(the spread) beside it.  Bytes a rotation needs: the map in and out, 2 N M F 4; the rate is these bytes over the time, against the
6.3 TB/s an MI355X reaches from HBM.  Outputs are compared (1e-6 max|x|) before anything is timed.

THE RULE the figures feed (healpy_layers._rotate_on_table): for a layer with a FIXED rotation, a channel count F goes to the cached
table through ell_smooth where that route is ahead of the kernel by more than the kernel's own spread over its three runs; the
verdict per shape is printed.  Prints the figures and one JSON line.  Needs a GPU: there is no CPU fallback and no figure without one.
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deepsphere-cosmo-tf2_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from deepsphere import _native, healpix  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes / s
RUNS = 3


def timed(fn, reps):
    """ms per call of `reps` back-to-back calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nside", type=int, default=1024)
    ap.add_argument("--shapes", default="8x1,4x4,4x16,2x64", help="N x F, comma separated")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-nside", type=int, default=256)
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    _native.require_gpu()
    dev = torch.device("cuda", 0)
    nside, M = args.nside, 12 * args.nside * args.nside
    gen = torch.Generator(device=dev).manual_seed(0)
    results = []
    for N, F in shapes:
        x = torch.randn((N, M, F), generator=gen, device=dev)
        alg = 2 * N * M * F * 4
        for shared in (False, True):
            rot = healpix.random_rotations(1 if shared else N, generator=gen, device=dev)
            rot = rot[0].contiguous() if shared else rot
            # the tables, built beforehand and timed on their own
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tables = [_native.healpix_interp_table(nside, r.contiguous()) for r in rot.reshape(-1, 3, 3)]
            torch.cuda.synchronize()
            build_ms = (time.perf_counter() - t0) * 1e3
            cols64 = [c.to(torch.int64) for c, _ in tables]
            table_bytes = sum(c.numel() * 4 + v.numel() * 4 for c, v in tables)
            outs = {name: torch.empty_like(x) for name in ("kernel", "ell_smooth", "torch")}

            def run_kernel():
                _native.healpix_rotate(x, nside, rot, out=outs["kernel"])

            def run_ell():
                if shared:
                    _native.ell_smooth(*tables[0], x, out=outs["ell_smooth"])
                else:
                    for n in range(N):
                        _native.ell_smooth(*tables[n], x[n:n + 1], out=outs["ell_smooth"][n:n + 1])

            def run_torch():
                for n in range(N):
                    (c, v), c64 = tables[0 if shared else n], cols64[0 if shared else n]
                    acc = x[n].index_select(0, c64[:, 0]) * v[:, 0:1]
                    for j in (1, 2, 3):
                        acc += x[n].index_select(0, c64[:, j]) * v[:, j:j + 1]
                    outs["torch"][n] = acc

            cases = {"kernel": run_kernel, "ell_smooth": run_ell, "torch": run_torch}
            for fn in cases.values():  # same numbers first (faster and different is not faster)
                fn()
            torch.cuda.synchronize()
            tol = 1e-6 * float(x.abs().max())
            for name in ("ell_smooth", "torch"):
                err = float((outs[name] - outs["kernel"]).abs().max())
                if not err <= tol:
                    raise SystemExit(f"N {N} F {F} shared {shared}: {name} differs from the kernel by {err:.3e} (tolerance {tol:.3e})")
            for _ in range(args.warmup):
                for fn in cases.values():
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name in cases}
            for _ in range(RUNS):  # alternating: drift of the machine hits every route alike
                for name, fn in cases.items():
                    times[name].append(timed(fn, args.reps))
            ms = {name: statistics.median(t) for name, t in times.items()}
            spread = max(times["kernel"]) - min(times["kernel"])
            to_table = shared and ms["kernel"] - ms["ell_smooth"] > spread
            kind = "one rotation for the batch" if shared else "a rotation per sample"
            print(f"nside {nside}, N {N}, F {F}, {kind}: {alg / 1e9:.3f} GB in and out; {len(tables)} table(s) of W = 4: "
                  f"{table_bytes / 1e6:.0f} MB (+ {sum(c.numel() * 8 for c in cols64) / 1e6:.0f} MB int64 columns for torch), "
                  f"built in {build_ms:.2f} ms")
            for name in cases:
                rate = alg / (ms[name] * 1e-3)
                print(f"  {name:11s} {ms[name]:9.4f} ms  (min {min(times[name]):.4f}, max {max(times[name]):.4f}; {RUNS} runs of "
                      f"{args.reps} calls)  {rate / 1e12:5.2f} TB/s = {rate / HBM_ACHIEVABLE:.2f} of {HBM_ACHIEVABLE / 1e12:.1f} TB/s", flush=True)
            if shared:
                print(f"  rule: kernel - ell_smooth = {ms['kernel'] - ms['ell_smooth']:+.4f} ms against the kernel's spread {spread:.4f} ms"
                      f" -> F = {F} {'goes to the table' if to_table else 'stays on the kernel'}")
            results.append({"N": N, "F": F, "shared_rotation": shared, "bytes": alg, "ms": ms,
                            "min_ms": {n: min(t) for n, t in times.items()}, "max_ms": {n: max(t) for n, t in times.items()},
                            "hbm_fraction": {n: alg / (ms[n] * 1e-3) / HBM_ACHIEVABLE for n in ms},
                            "table_bytes": table_bytes, "table_build_ms": build_ms, "fixed_rotation_to_table": to_table})
            del tables, cols64, outs
        del x
    # the host route, at its own nside: stencil and gather in numpy, then the copy
    hn, hm = args.host_nside, 12 * args.host_nside * args.host_nside
    N, F = shapes[0]
    xh = np.random.default_rng(0).standard_normal((N, hm, F)).astype(np.float32)
    rots = healpix.random_rotations(N, generator=torch.Generator().manual_seed(0)).numpy()
    vec = healpix.pix2vec(hn)
    host = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        out = np.empty_like(xh)
        for n in range(N):
            u = vec @ rots[n]
            out[n] = healpix.get_interp_val(xh[n].T, np.arctan2(np.hypot(u[:, 0], u[:, 1]), u[:, 2]), np.arctan2(u[:, 1], u[:, 0])).T
        torch.as_tensor(out).to(dev)
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
    print(f"host route, nside {hn}, N {N}, F {F}, a rotation per sample: {statistics.median(host):.1f} ms "
          f"(min {min(host):.1f}, max {max(host):.1f}; {RUNS} runs), {statistics.median(host) / N:.1f} ms a map of {hm} pixels")
    print(json.dumps({"nside": nside, "M": M, "reps": args.reps, "runs": RUNS, "results": results,
                      "host": {"nside": hn, "N": N, "F": F, "ms": statistics.median(host), "min_ms": min(host), "max_ms": max(host)}}))


if __name__ == "__main__":
    main()
