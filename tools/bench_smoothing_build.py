#!/usr/bin/env python3
"""Time the construction of HealpySmoothing with build="host" and build="device", and the first backward of each, on one box.

    python tools/bench_smoothing_build.py [--nside 128 512] [--factor 1.5] [--reps 3] [--footprint-nside 256] [--no-host]

Per shape, alternating host, device, host, ... `--reps` times each (drift of the machine hits both alike):
  build     wall time of the constructor; for the device build the device is synchronised before the clock stops
  backward  wall time of the first call of `_transposed_tables` with the table resident on the GPU, as the first backward finds
            it: the host route copies the table down, transposes it with scipy and copies it up, the device route sorts on the GPU
  kernels   (device) the two launches of csrc/healpix_disc.hip alone, by device events: their share of the build
  peak      (device) the torch allocator's high-water mark over constructor and transpose
Shapes: the full sky at every `--nside`, sigma = `--factor` x the pixel resolution sqrt(4 pi / npix), 3 sigma support; and one survey
footprint, the polar cap of a twentieth of the sky at `--footprint-nside` extended to whole nside-16 super-pixels (0: none).
Prints median, smallest and largest of every figure and one JSON line.  Needs a GPU.
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
from deepsphere.healpy_layers import HealpySmoothing  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def kernel_seconds(nside, indices, sigma, dev):
    """The two launches alone, by device events, with the arguments `healpix.gauss_table_device` gives them."""
    npix = 12 * nside * nside
    rho = min(3.0 * sigma, np.pi)
    ps = (None, None) if indices.shape[0] == npix else healpix._device_lut(nside, indices, dev)
    kw = {"device": dev} if ps[0] is None else {}
    a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    a.record()
    count, _ = _native.healpix_disc_count(nside, (2.0 * np.sin(0.5 * rho)) ** 2, *ps, **kw)
    b.record()
    W = int(count.max())
    out = _native.healpix_gauss_table(nside, W, sigma, rho, *ps, **kw)
    c.record()
    c.synchronize()
    del out
    return a.elapsed_time(b) * 1e-3, b.elapsed_time(c) * 1e-3


def one(build, nside, indices, sigma, dev):
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t_build, layer = wall(lambda: HealpySmoothing(nside, indices, sigma=sigma, arcmin=False, build=build))
    layer._tables(dev)  # (where the first forward leaves the table)
    t_back, tT = wall(lambda: layer._transposed_tables(dev))
    peak = torch.cuda.max_memory_allocated() - base
    res = {"build": t_build, "backward": t_back, "peak": peak, "W": layer.max_neighbors, "WT": int(tT[0].shape[1]),
           "completed": layer.completed}
    del layer, tT
    torch.cuda.empty_cache()
    return res


def summary(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nside", type=int, nargs="*", default=[128, 512])
    ap.add_argument("--factor", type=float, default=1.5, help="sigma in units of the pixel resolution")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--footprint-nside", type=int, default=256)
    ap.add_argument("--no-host", action="store_true", help="device build only")
    args = ap.parse_args()
    _native.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    shapes = [(f"full{n}", n, np.arange(12 * n * n, dtype=np.int64)) for n in args.nside]
    if args.footprint_nside:
        n = args.footprint_nside
        shapes.append((f"cap{n}", n, healpix.extend_indices(healpix.cap_indices(n, fraction=0.05), n, 16)))
    one("device", 8, np.arange(768), np.sqrt(4 * np.pi / 768), dev)  # (library and allocator warm)
    result = {}
    for name, nside, indices in shapes:
        sigma = args.factor * np.sqrt(4 * np.pi / (12 * nside * nside))
        runs = {"device": []} if args.no_host else {"host": [], "device": []}
        for rep in range(args.reps):
            for build in runs:
                r = one(build, nside, indices, sigma, dev)
                runs[build].append(r)
                print(f"{name} {build} #{rep}: build {r['build']:.3f} s, first backward {r['backward']:.3f} s, W {r['W']}, WT {r['WT']}, "
                      f"completed {r['completed']}", flush=True)
        kern = [kernel_seconds(nside, indices, sigma, dev) for _ in range(args.reps)]
        entry = {"M": int(indices.shape[0]), "W": runs["device"][0]["W"], "completed": runs["device"][0]["completed"],
                 "kernels_s": {"count": summary([k[0] for k in kern]), "table": summary([k[1] for k in kern])},
                 "device_peak_bytes": max(r["peak"] for r in runs["device"])}
        for build, rs in runs.items():
            entry[build] = {"build_s": summary([r["build"] for r in rs]), "backward_s": summary([r["backward"] for r in rs])}
        result[name] = entry
        for build in runs:
            b, t = entry[build]["build_s"], entry[build]["backward_s"]
            print(f"{name:8s} {build:6s} build {b['median']:9.3f} s ({b['min']:.3f} .. {b['max']:.3f})   first backward {t['median']:9.3f} s "
                  f"({t['min']:.3f} .. {t['max']:.3f})")
        k = entry["kernels_s"]
        print(f"{name:8s} kernels: count {k['count']['median'] * 1e3:.2f} ms, table {k['table']['median'] * 1e3:.2f} ms = "
              f"{(k['count']['median'] + k['table']['median']) / entry['device']['build_s']['median']:.2f} of the device build; "
              f"peak device memory of the device build {entry['device_peak_bytes'] / 2**30:.2f} GiB "
              f"(table {8 * entry['M'] * entry['W'] / 2**30:.2f} GiB)", flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
