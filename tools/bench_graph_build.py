#!/usr/bin/env python3
"""Time the construction of HealpyGCNN with its graphs built on the host and on the device, on one GPU.

    python tools/bench_graph_build.py [--model-nside 256] [--k 20] [--graph-nsides 512,1024] [--reps 5] [--host-reps 2]
                                      [--host-graph-max-nside 1024]

(model)  HealpyGCNN(nside, full sky, [HealpyChebyshev(K=5, Fout=8), HealpyPool(1), HealpyChebyshev(K=5, Fout=8)], n_neighbors=k)
         with build="host" (k-d tree, csr.maximum, ARPACK eigsh at machine precision, csr_to_ell: once per graph layer) and with
         build="device" (HIP k-NN kernel, torch assembly, Lanczos lmax), at one resolution where the host path still finishes;
(graph)  the device graph alone (healpix.healpix_laplacian_ell, mode="knn") against healpix.healpix_graph on the host, and the
         device's high-water mark of allocated memory during it (torch.cuda.max_memory_allocated).
(diff)   the output difference between a host-built and a device-built network with identical weights, grid mode at nside 16,
         lmax from Lanczos on the device side: max |y_dev - y_host| / max |y_host|.  Recorded, not asserted.
Host clocks around work that ends in a device synchronise; every route once before anything is timed (code objects, torch's
caches); median with smallest and largest beside it.  The host routes take minutes: --host-reps repeats of them (one at the largest
nside by default is all a GPU session affords; its spread is then "not measured").  Prints the figures and one JSON line.  Needs a
GPU: no figure without one."""

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
from deepsphere.healpy_layers import HealpyChebyshev, HealpyPool  # noqa: E402
from deepsphere.healpy_networks import HealpyGCNN  # noqa: E402


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def summary(times):
    return {"median_s": statistics.median(times), "min_s": min(times), "max_s": max(times), "reps": len(times)}


def show(name, s):
    spread = f"min {s['min_s']:.3f}, max {s['max_s']:.3f}" if s["reps"] > 1 else "one run: spread not measured"
    print(f"  {name:28s} {s['median_s']:9.3f} s  ({spread}, {s['reps']} runs)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-nside", type=int, default=256)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--graph-nsides", default="512,1024")
    ap.add_argument("--reps", type=int, default=5, help="repeats of the device routes")
    ap.add_argument("--host-reps", type=int, default=2, help="repeats of the host routes below the largest nside")
    ap.add_argument("--host-graph-max-nside", type=int, default=1024, help="the host graph is not built above this nside")
    args = ap.parse_args()
    _native.require_gpu()
    dev = torch.device("cuda", 0)
    k = args.k
    result = {"k": k}

    def layers():
        return [HealpyChebyshev(K=5, Fout=8), HealpyPool(1), HealpyChebyshev(K=5, Fout=8)]

    # warm-up: every route once at a small size
    for build in ("host", "device"):
        HealpyGCNN(16, np.arange(3072), layers(), n_neighbors=k, build=build)
    healpix.healpix_laplacian_ell(32, None, k, "knn", device=dev)

    if args.model_nside > 0:
        nside = args.model_nside
        ind = np.arange(12 * nside * nside)
        print(f"model: HealpyGCNN(nside {nside}, full sky, Chebyshev - Pool - Chebyshev, n_neighbors {k})", flush=True)
        times = {"device": [], "host": []}
        for r in range(max(args.reps, args.host_reps)):  # alternating
            for build, reps in (("device", args.reps), ("host", args.host_reps)):
                if r < reps:
                    times[build].append(clocked(lambda: HealpyGCNN(nside, ind, layers(), n_neighbors=k, build=build))[0])
                    print(f"  run {r} build=\"{build}\": {times[build][-1]:.3f} s", flush=True)
        result["model"] = {"nside": nside, **{b: summary(t) for b, t in times.items()}}
        for b in ("host", "device"):
            show(f"build=\"{b}\"", result["model"][b])

    result["graph"] = []
    nsides = [int(v) for v in args.graph_nsides.split(",") if v]
    for nside in nsides:
        print(f"graph: nside {nside}, k {k}, full sky ({12 * nside * nside} pixels)")
        entry = {"nside": nside}
        healpix.healpix_laplacian_ell(nside, None, k, "knn", device=dev)  # (this size once: allocator, code paths)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        dt = []
        for _ in range(args.reps):
            t, out = clocked(lambda: healpix.healpix_laplacian_ell(nside, None, k, "knn", device=dev))
            dt.append(t)
            width = int(out[0].shape[1])
            del out
        entry["device_laplacian_ell"] = summary(dt)
        entry["device_peak_allocated_GB"] = torch.cuda.max_memory_allocated(dev) / 1e9
        entry["ell_width"] = width
        show("device healpix_laplacian_ell", entry["device_laplacian_ell"])
        print(f"  device high-water mark of allocated memory: {entry['device_peak_allocated_GB']:.2f} GB (ELL width {width})")
        kt = []
        for _ in range(args.reps):
            kt.append(clocked(lambda: _native.healpix_knn(nside, k, device=dev))[0])
        entry["device_knn_kernel"] = summary(kt)
        show("  of it: dsph_healpix_knn", entry["device_knn_kernel"])
        if nside <= args.host_graph_max_nside:
            reps = args.host_reps if nside < max(nsides) else 1
            ht = [clocked(lambda: healpix.healpix_graph(nside, None, k, "knn"))[0] for _ in range(reps)]
            entry["host_healpix_graph"] = summary(ht)
            show("host healpix_graph", entry["host_healpix_graph"])
        result["graph"].append(entry)

    # host-built against device-built, identical weights: grid mode (no ties), lmax from Lanczos on the device side
    spec = [HealpyChebyshev(K=5, Fout=8, precision="fp32", use_bias=True, activation="relu")]
    host = HealpyGCNN(16, np.arange(3072), spec, graph_mode="grid", build="host")
    devm = HealpyGCNN(16, np.arange(3072), spec, graph_mode="grid", build="device")
    x = torch.randn(2, 3072, 4, generator=torch.Generator().manual_seed(0)).to(dev)
    with torch.no_grad():
        yh = host(x)
        devm(x)
        devm.load_state_dict(host.state_dict())
        yd = devm(x)
    result["diff"] = {"lmax_host": host[0].lmax, "lmax_device": devm[0].lmax,
                      "lmax_rel": abs(devm[0].lmax - host[0].lmax) / host[0].lmax,
                      "y_rel": float((yd - yh).abs().max() / yh.abs().max())}
    print(f"diff: grid, nside 16, K 5: lmax host {host[0].lmax!r} device {devm[0].lmax!r} (rel {result['diff']['lmax_rel']:.3g}), "
          f"max |y_dev - y_host| / max |y_host| = {result['diff']['y_rel']:.3g}")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
