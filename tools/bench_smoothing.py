#!/usr/bin/env python3
"""Time one pass of HealpySmoothing against two other routes over the same kernel table, on one GPU.

    python tools/bench_smoothing.py [--nside 512] [--factor 1.5] [--batch 8] [--channels 4] [--reps 20] [--warmup 3] [--no-sparse] [--build host|device]

(layer) the layer's forward: one launch of dsph_ell_smooth (a group of lanes per row, the table read once per pass);
(a) the only route the library had before: _native.cheb_step on a LaplacianPlan built from the same table (alpha = 1, no
    prev): one thread per (row, channel vector), the row's entries walked one after another;
(b) the reference's formulation in torch on the same device: per channel, torch.sparse.mm of the (M, M) CSR matrix with the
    (M, N) slice, with the transposes and the stack around it.
Default shape: full sky at nside 512, sigma = 1.5 x the pixel resolution sqrt(4 pi / npix), 3 sigma support, N = 8, C = 4: rows of
about 70 entries and a table of about 1.8 GB.  All routes run in this process, alternating, after a warm-up; times are medians
of device-event timings of single calls, with the smallest and largest beside them.  Bytes a pass needs: the table once and the
map in and out, 8 W M + 8 N M C; the rate is these bytes over the layer's time, against the 6.3 TB/s an MI355X reaches from HBM.
Peak memory is the torch allocator's high-water mark over a call, the operands (maps, tables) excluded; the tables' sizes are
printed beside it.  Prints the figures and one JSON line.  Needs a GPU: there is no CPU fallback and no figure without one.
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

from deepsphere import _native  # noqa: E402
from deepsphere.healpy_layers import HealpySmoothing  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes / s


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def peak_over(fn):
    """Bytes the torch allocator holds at most during one call, above what it held before."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nside", type=int, default=512)
    ap.add_argument("--factor", type=float, default=1.5, help="sigma in units of the pixel resolution")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--channels", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-sparse", action="store_true", help="leave route (b) out")
    ap.add_argument("--build", choices=("host", "device"), default="host", help="where the layer builds its table")
    args = ap.parse_args()
    _native.require_gpu()
    dev = torch.device("cuda", 0)
    npix = 12 * args.nside * args.nside
    t0 = time.time()
    layer = HealpySmoothing(args.nside, np.arange(npix), sigma=args.factor * np.sqrt(4 * np.pi / npix), arcmin=False, build=args.build)
    M, W, N, C = npix, layer.max_neighbors, args.batch, args.channels
    print(f"nside {args.nside}: M {M}, W {W}, table {8 * W * M / 1e9:.2f} GB, built on the {args.build} in {time.time() - t0:.0f} s", flush=True)
    t0 = time.time()
    plan = _native.LaplacianPlan(layer.cols.cpu().numpy(), layer.vals.cpu().numpy(), device=0)
    print(f"route (a): plan of the same table created in {time.time() - t0:.0f} s", flush=True)
    cols, vals = layer._tables(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((N, M, C), generator=gen, device=dev)

    def run_layer():
        with torch.no_grad():
            return layer(x)

    def run_step():
        return _native.cheb_step(plan, x, None, 1.0, 0.0)

    cases = {"layer": run_layer, "cheb_step": run_step}
    table_bytes = {"layer": 8 * W * M, "cheb_step": 8 * W * M}
    if not args.no_sparse:
        crow = torch.arange(0, M * W + 1, W, dtype=torch.int64, device=dev)
        K = torch.sparse_csr_tensor(crow, cols.reshape(-1).to(torch.int64), vals.reshape(-1), size=(M, M))
        table_bytes["sparse_mm"] = 8 * (M + 1) + 12 * W * M

        def run_sparse():
            with torch.no_grad():
                first = x.permute(1, 0, 2)  # (M, N, C), the reference's transposes
                return torch.stack([torch.sparse.mm(K, first[:, :, c].contiguous()) for c in range(C)], dim=2).permute(1, 0, 2).contiguous()

        cases["sparse_mm"] = run_sparse

    # same numbers first (faster and different is not faster)
    want = run_layer()
    agree = {name: float((fn() - want).abs().max() / want.abs().max()) for name, fn in cases.items() if name != "layer"}
    del want
    peak = {name: peak_over(fn) for name, fn in cases.items()}
    for _ in range(args.warmup):
        for fn in cases.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in cases}
    for _ in range(args.reps):  # alternating: drift of the machine hits every case alike
        for name, fn in cases.items():
            times[name].append(timed(fn))
    ms = {name: statistics.median(t) for name, t in times.items()}
    spread = {name: (min(t), max(t)) for name, t in times.items()}
    alg = 8 * W * M + 8 * N * M * C
    rate = alg / (ms["layer"] * 1e-3)
    print(f"batch {N}, {C} channels, one pass; agreement with the layer (max rel): " + ", ".join(f"{n} {e:.1e}" for n, e in agree.items()))
    for name in cases:
        print(f"{name:10s} {ms[name]:9.3f} ms   (min {spread[name][0]:.3f}, max {spread[name][1]:.3f}, {args.reps} calls)   "
              f"peak {peak[name] / 2**20:8.1f} MiB beside a table of {table_bytes[name] / 1e9:.2f} GB")
    print(f"layer: {alg / 1e9:.3f} GB per pass, {rate / 1e12:.2f} TB/s = {rate / HBM_ACHIEVABLE:.2f} of {HBM_ACHIEVABLE / 1e12:.1f} TB/s")
    print("layer against: " + ", ".join(f"{n} {ms[n] / ms['layer']:.2f} x" for n in cases if n != "layer"))
    print(json.dumps({"nside": args.nside, "build": args.build, "M": M, "W": W, "batch": N, "channels": C, "ms": ms, "spread_ms": spread,
                      "peak_bytes": peak, "table_bytes": table_bytes, "bytes_per_pass": alg,
                      "hbm_fraction": rate / HBM_ACHIEVABLE, "agreement": agree}))


if __name__ == "__main__":
    main()
