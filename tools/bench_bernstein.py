#!/usr/bin/env python3
"""Time a Bernstein layer of order K against the Chebyshev layer with K + 1 terms it runs as, on one GPU.

    python tools/bench_bernstein.py [--nside 256] [--batch 8] [--fin 64] [--fout 64] [--K 5] [--reps 30] [--warmup 5]

Two claims of DESIGN.md rest on these numbers: that ``Bernstein(K)`` costs what ``Chebyshev(K + 1)`` costs at inference (the
transformed weights are cached: the steady state launches nothing extra), and that a training step adds two small launches
(``dsph_basis_change`` on the weights going in and on the weight gradient coming out).  The baseline is the Chebyshev layer:
kernels this tool's subject does not touch.  Timed, on the full-sky 8-neighbour graph of bench.py:
  (inference)  ``layer(x)`` under ``torch.no_grad()``, both layers, after the warm-up has packed the weight images;
  (training)   forward plus backward (``y = layer(x); y.backward(dy)``; gradients of x and of the kernel), both layers;
  (basis)      ``dsph_basis_change`` alone on the layer's [(K + 1) Fin, Fout] weights, both directions.
All in this process, alternating, after a warm-up; times are medians of device-event timings of single calls with the smallest
and largest beside them.  The Chebyshev layer holds the Bernstein layer's weights in its own basis, so the two inference
outputs must be the same bits: checked before anything is timed.  Sets no threshold.  Prints the figures and one JSON line.
Needs a GPU: there is no CPU fallback and no figure without one.
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

import bench  # noqa: E402
from deepsphere import _native  # noqa: E402
from deepsphere.gnn_layers import Bernstein, Chebyshev, bernstein_to_chebyshev  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(cases, warmup, reps):
    """{name: fn} -> {name: (median ms, min, max)}; the cases take turns, so drift of the machine hits them alike."""
    for _ in range(warmup):
        for fn in cases.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in cases}
    for _ in range(reps):
        for name, fn in cases.items():
            times[name].append(timed(fn))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nside", type=int, default=256)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--fin", type=int, default=64)
    ap.add_argument("--fout", type=int, default=64)
    ap.add_argument("--K", type=int, default=5, help="order of the Bernstein layer; the Chebyshev layer has K + 1 terms")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    _native.require_gpu()
    dev = torch.device("cuda", 0)
    K, Fin, Fout, N = args.K, args.fin, args.fout, args.batch
    cols, vals, _ = bench.build_laplacian(args.nside, dev)
    M = cols.shape[0]
    torch.manual_seed(0)
    bern = Bernstein.from_prepared_ell(cols, vals, K, Fout=Fout, device=dev)
    cheb = Chebyshev.from_prepared_ell(cols, vals, K + 1, Fout=Fout, device=dev)
    bern.build((N, M, Fin))
    cheb.build((N, M, Fin))
    C = torch.as_tensor(bernstein_to_chebyshev(K).astype(np.float32)).to(dev)
    with torch.no_grad():
        cheb.kernel.copy_(_native.basis_change(bern.kernel.detach(), C))
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((N, M, Fin), generator=gen, device=dev)
    dy = torch.randn((N, M, Fout), generator=gen, device=dev)
    print(f"nside {args.nside}: M {M}, batch {N}, {Fin} -> {Fout}, Bernstein K = {K} against Chebyshev with {K + 1} terms", flush=True)

    def inference(layer):
        def run():
            with torch.no_grad():
                return layer(x)
        return run

    def training(layer):
        xg = x.clone().requires_grad_(True)

        def run():
            xg.grad = None
            layer.kernel.grad = None
            layer(xg).backward(dy)
        return run

    # same numbers first (faster and different is not faster)
    same = bool(torch.equal(inference(bern)(), inference(cheb)()))
    print(f"inference outputs are the same bits: {same}", flush=True)
    inf = alternate({"bernstein": inference(bern), "chebyshev": inference(cheb)}, args.warmup, args.reps)
    rebuilds = bern._basis_image["count"]
    trn = alternate({"bernstein": training(bern), "chebyshev": training(cheb)}, args.warmup, args.reps)
    w = bern.kernel.detach()
    out = torch.empty_like(w)
    bas = alternate({"in": lambda: _native.basis_change(w, C, out=out),
                     "out": lambda: _native.basis_change(w, C, transpose=True, out=out)}, args.warmup, args.reps)
    for title, res in (("inference", inf), ("forward + backward", trn), ("dsph_basis_change", bas)):
        for name, (med, lo, hi) in res.items():
            print(f"{title:20s} {name:10s} {med:9.4f} ms   (min {lo:.4f}, max {hi:.4f}, {args.reps} calls)")
    print(f"Bernstein / Chebyshev: inference {inf['bernstein'][0] / inf['chebyshev'][0]:.3f}, "
          f"forward + backward {trn['bernstein'][0] / trn['chebyshev'][0]:.3f}; weight images rebuilt {rebuilds} time(s) at inference")
    print(json.dumps({"nside": args.nside, "M": M, "batch": N, "Fin": Fin, "Fout": Fout, "K": K, "same_bits": same,
                      "inference_ms": inf, "training_ms": trn, "basis_change_ms": bas, "inference_rebuilds": rebuilds}))


if __name__ == "__main__":
    main()
