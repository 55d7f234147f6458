#!/usr/bin/env python3
"""Time a training-mode batch-norm layer on the batch-norm kernels against the composition they replace, on one GPU.

    python tools/bench_batchnorm.py [--shapes headline,c2,quickstart] [--reps 10] [--warmup 3]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_batchnorm.py --profile headline      (kernel times, a run of its own)
    python tools/bench_batchnorm.py --kernel-stats DIR --profile headline                              (bytes/s from that run)

The layer is ``Chebyshev(K=5, use_bn=True, use_bias=True, activation="relu")`` called as ``layer(x, training=True)``.  Two paths:
  (new)     the layer as it is: convolution, then ``dsph_bn_stats`` + ``dsph_bn_apply`` (backward: ``dsph_bn_backward``);
  (parent)  the composition the layer ran before, written out here: the same convolution through a twin layer without epilogue,
            then ``torch.nn.functional.batch_norm`` on the transposed view, ``+ bias``, ``relu``.
Both in this process, taking turns after a warm-up, each call between two device events; medians with the smallest and largest
beside them (the spread of a path against itself).  Measured: the forward under ``torch.no_grad()``, and forward + backward (gradients of x, kernel and
bias), with ``torch.cuda.max_memory_allocated`` of each path's forward + backward.  The two outputs are compared first.  Shapes:
  headline    nside 1024, batch 4, 64 -> 64   (BASELINE.json configs[2])
  c2          nside 256, batch 8, 16 -> 32    (BASELINE.json configs[1])
  quickstart  nside 64, batch 16, 1 -> 5      (a narrow layer like the reference's quick-start model's)
Sets no threshold.  Prints the figures and one JSON line per shape.  Needs a GPU: there is no CPU fallback and no figure without one.

``--profile SHAPE`` runs forward + backward of the new path a few times and nothing else, to be traced; ``--kernel-stats DIR``
reads the ``kernel_stats.csv`` of such a trace and prints the achieved bytes/s of the ``bn_*`` kernels: the three forward passes
(statistics: one read; apply: one read, one write) and the seven backward ones (reduction: three reads; gradient: three reads,
one write) of 4 * rows * F bytes each.
"""

import argparse
import csv
import glob
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deepsphere-cosmo-tf2_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench  # noqa: E402
from deepsphere import _native  # noqa: E402
from deepsphere.gnn_layers import Chebyshev  # noqa: E402

SHAPES = {"headline": (1024, 4, 64, 64), "c2": (256, 8, 16, 32), "quickstart": (64, 16, 1, 5)}  # nside, batch, Fin, Fout
K = 5
# passes over the (rows, F) map per kernel: (reads, writes)
PASSES = {"bn_stats_partial_kernel": (1, 0), "bn_apply_kernel": (1, 1), "bn_bwd_partial_kernel": (3, 0), "bn_bwd_apply_kernel": (3, 1)}


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


def build(shape, dev):
    nside, N, Fin, Fout = SHAPES[shape]
    cols, vals, _ = bench.build_laplacian(nside, dev)
    M = cols.shape[0]
    torch.manual_seed(0)
    layer = Chebyshev.from_prepared_ell(cols, vals, K, Fout=Fout, use_bn=True, use_bias=True, activation="relu", device=dev)
    twin = Chebyshev.from_prepared_ell(cols, vals, K, Fout=Fout, device=dev)  # the convolution alone
    layer.build((N, M, Fin))
    twin.build((N, M, Fin))
    with torch.no_grad():
        twin.kernel.copy_(layer.kernel)
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((N, M, Fin), generator=gen, device=dev)
    dy = torch.randn((N, M, Fout), generator=gen, device=dev)
    return layer, twin, x, dy, M


def paths(layer, twin, x, dy):
    """-> {"new": (forward, forward + backward), "parent": (...)}; every closure returns its output (or None)."""
    bias_p = layer.bias.detach().clone().requires_grad_(True)
    rm, rv = layer.bn.running_mean.clone(), layer.bn.running_var.clone()
    eps, momentum = layer.bn.eps, layer.bn.momentum

    def parent(inp):
        c = twin(inp)
        y = torch.nn.functional.batch_norm(c.transpose(1, 2), rm, rv, None, None, True, momentum, eps).transpose(1, 2)
        return torch.relu(y + bias_p)

    def new_fwd():
        with torch.no_grad():
            return layer(x, training=True)

    def parent_fwd():
        with torch.no_grad():
            return parent(x)

    xg = x.clone().requires_grad_(True)

    def new_step():
        xg.grad = layer.kernel.grad = layer.bias.grad = None
        layer(xg, training=True).backward(dy)

    def parent_step():
        xg.grad = twin.kernel.grad = bias_p.grad = None
        parent(xg).backward(dy)

    return {"new": (new_fwd, new_step), "parent": (parent_fwd, parent_step)}


def peak_memory(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def measure(shape, dev, warmup, reps):
    nside, N, Fin, Fout = SHAPES[shape]
    layer, twin, x, dy, M = build(shape, dev)
    p = paths(layer, twin, x, dy)
    print(f"{shape}: nside {nside}, M {M}, batch {N}, {Fin} -> {Fout}, K = {K}; one pass over the output map is {4 * N * M * Fout / 1e9:.3f} GB",
          flush=True)
    a, b = p["new"][0](), p["parent"][0]()
    diff = float((a - b).abs().max() / b.abs().max())
    del a, b
    print(f"  outputs of the two paths: max |difference| / max |y| = {diff:.2e}", flush=True)
    fwd = alternate({name: fns[0] for name, fns in p.items()}, warmup, reps)
    step = alternate({name: fns[1] for name, fns in p.items()}, warmup, reps)
    with torch.no_grad():
        conv = alternate({"conv": lambda: twin(x)}, 1, reps)["conv"]
    mem = {name: peak_memory(fns[1]) for name, fns in p.items()}
    for title, res in (("forward", fwd), ("forward + backward", step)):
        for name, (med, lo, hi) in res.items():
            print(f"  {title:20s} {name:8s} {med:10.4f} ms   (min {lo:.4f}, max {hi:.4f}, {reps} calls)")
        print(f"  {title:20s} parent / new = {res['parent'][0] / res['new'][0]:.3f}")
    print(f"  {'convolution alone':20s} {'':8s} {conv[0]:10.4f} ms   (forward, no epilogue)")
    print(f"  peak memory of forward + backward above the resident tensors: new {mem['new'] / 2**20:.1f} MiB, parent {mem['parent'] / 2**20:.1f} MiB")
    print(json.dumps({"shape": shape, "nside": nside, "M": M, "batch": N, "Fin": Fin, "Fout": Fout, "K": K, "output_difference": diff,
                      "forward_ms": fwd, "forward_backward_ms": step, "conv_forward_ms": conv, "peak_bytes": mem}), flush=True)


def profile(shape, dev, steps=5):
    layer, twin, x, dy, _ = build(shape, dev)
    _, step = paths(layer, twin, x, dy)["new"]
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    print(f"profile run: {steps} training steps of the new path at {shape}")


def kernel_stats(directory, shape):
    nside, N, _, Fout = SHAPES[shape]
    map_bytes = 4 * N * 12 * nside * nside * Fout
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel_stats.csv under {directory}")
    out = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            for key, (reads, writes) in PASSES.items():
                if key in r["Name"]:
                    avg_ms = float(r["AverageNs"]) / 1e6
                    out[key] = {"calls": int(r["Calls"]), "avg_ms": avg_ms, "passes": reads + writes,
                                "TB_per_s": (reads + writes) * map_bytes / (avg_ms * 1e-3) / 1e12}
            for key in ("bn_stats_final_kernel", "bn_bwd_final_kernel"):
                if key in r["Name"]:
                    out[key] = {"calls": int(r["Calls"]), "avg_ms": float(r["AverageNs"]) / 1e6}
    print(f"{shape}: one pass over the map is {map_bytes / 1e9:.3f} GB")
    for key, v in out.items():
        extra = f"{v['passes']} passes, {v['TB_per_s']:.2f} TB/s" if "passes" in v else "the fixed-order merge of the partials"
        print(f"  {key:26s} {v['calls']:4d} calls, {v['avg_ms']:9.4f} ms each   ({extra})")
    print(json.dumps({"shape": shape, "map_bytes": map_bytes, "kernels": out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,c2,quickstart")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile", metavar="SHAPE", default=None, choices=sorted(SHAPES))
    ap.add_argument("--kernel-stats", metavar="DIR", default=None)
    args = ap.parse_args()
    if args.kernel_stats:
        kernel_stats(args.kernel_stats, args.profile or "headline")
        return
    _native.require_gpu()
    dev = torch.device("cuda", 0)
    if args.profile:
        profile(args.profile, dev)
        return
    for shape in args.shapes.split(","):
        measure(shape, dev, args.warmup, args.reps)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
