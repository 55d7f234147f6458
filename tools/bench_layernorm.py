#!/usr/bin/env python3
"""Time the layer-norm kernels, and the layers on them, against the torch composition they replace, on one GPU.

    python tools/bench_layernorm.py [--shapes gt256,gt64,vit,res256] [--reps 10] [--warmup 3]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_layernorm.py --profile gt256       (kernel times, a run of its own)
    python tools/bench_layernorm.py --kernel-stats DIR --profile gt256                               (bytes/s from that run)

Two levels per shape, both paths in this process, taking turns after a warm-up, each call between two device events; medians with
the smallest and largest beside them (the spread of a path against itself):
  (a) add + layer norm alone: ``_LayerNormFunction`` (``dsph_ln_forward`` / ``dsph_ln_backward``) against ``x + res`` and
      ``torch.nn.functional.layer_norm``; forward under ``torch.no_grad()``, and forward + backward with both outputs used (gradients
      of x, res, weight and bias).  The residual block has no add in front of its norms: there the norm alone.
  (b) one whole block as it is now against the parent's composition written out here around the same attention call (the same
      convolutions for the residual block): torch's two layer norms, ``x + att``, the activation and ``+ att`` as separate passes.
Shapes:
  gt256    Graph_Transformer block, nside 256 full sky (8-neighbour graph), batch 4, 4 heads x 16
  gt64     the same at nside 64, batch 8, 2 heads x 8
  vit      Graph_ViT block, 3,072 tokens, batch 8, 4 heads x 32 (dense attention)
  res256   GCNN_ResidualLayer("CHEBY", K = 5, norm_type="layer_norm"), nside 256, batch 8, F = 32
Sets no threshold.  Prints the figures and one JSON line per shape and level.  Needs a GPU: there is no figure without one.

``--profile SHAPE`` runs forward + backward of level (a) on the kernels a few times and nothing else, to be traced;
``--kernel-stats DIR`` reads the ``kernel_stats.csv`` of such a trace and prints the achieved bytes/s of the two row kernels: with
the add, the forward reads two maps and writes two, the backward reads three and writes one, 4 * rows * d bytes each.
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

from deepsphere import _native, gnn_layers, gnn_transformers, healpix  # noqa: E402
from deepsphere.gnn_layers import GCNN_ResidualLayer, _LayerNormFunction  # noqa: E402

# kind, nside or tokens, batch, heads, depth (residual: F in the place of heads, depth 1)
SHAPES = {"gt256": ("sparse", 256, 4, 4, 16), "gt64": ("sparse", 64, 8, 2, 8), "vit": ("dense", 3072, 8, 4, 32),
          "res256": ("residual", 256, 8, 32, 1)}
EPS = 1e-3
RES_K = 5
# passes over the (rows, d) map per kernel: (reads, writes), with and without the add / dsum
PASSES = {"ln_fwd_kernel": {True: (2, 2), False: (1, 1)}, "ln_bwd_kernel": {True: (3, 1), False: (2, 1)}}


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


def peak_memory(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def grid_neighbour_table(nside, dev):
    """The neighbour table of the 8-neighbour HEALPix graph (symmetric: its own transpose), built on the device."""
    cols, _ = healpix.grid_laplacian_ell_torch(nside, device=dev)
    own = cols[:, :1].to(torch.int64)
    nb = cols[:, 1:].to(torch.int64)
    nb = torch.where(nb == own, torch.full_like(nb, 2**31 - 1), nb).sort(dim=1).values  # (a missing neighbour is stored as the pixel itself)
    return torch.where(nb == 2**31 - 1, torch.full_like(nb, -1), nb).to(torch.int32).contiguous()


def dims(shape):
    kind, size, N, heads, depth = SHAPES[shape]
    M = 12 * size * size if kind != "dense" else size
    return kind, N, M, heads * depth


def level_a(shape, dev):
    """-> {"new": (forward, step), "parent": (...)}, with_res"""
    kind, N, M, d = dims(shape)
    with_res = kind != "residual"
    gen = torch.Generator(device=dev).manual_seed(0)
    x, res, dz, dsum = (torch.randn((N, M, d), generator=gen, device=dev) for _ in range(4))
    x += 3.0
    w = (1.0 + 0.2 * torch.randn(d, generator=gen, device=dev)).requires_grad_(True)
    b = (0.3 * torch.randn(d, generator=gen, device=dev)).requires_grad_(True)
    xg, rg = x.clone().requires_grad_(True), res.clone().requires_grad_(True)

    def new(a, r):
        return _LayerNormFunction.apply(a, r if with_res else None, w, b, EPS)

    def parent(a, r):
        if not with_res:
            return torch.nn.functional.layer_norm(a, (d,), w, b, EPS)
        s = a + r
        return torch.nn.functional.layer_norm(s, (d,), w, b, EPS), s

    def forward(f):
        def run():
            with torch.no_grad():
                return f(x, res)
        return run

    def step(f):
        def run():
            xg.grad = rg.grad = w.grad = b.grad = None
            out = f(xg, rg)
            if with_res:
                torch.autograd.backward(list(out), [dz, dsum])
            else:
                out.backward(dz)
        return run

    return {"new": (forward(new), step(new)), "parent": (forward(parent), step(parent))}, with_res


def level_b(shape, dev):
    kind, size, N, heads, depth = SHAPES[shape]
    _, _, M, d = dims(shape)
    gen = torch.Generator(device=dev).manual_seed(1)
    torch.manual_seed(1)
    if kind == "residual":
        L = healpix.healpix_laplacian(size, mode="grid")
        block = GCNN_ResidualLayer("CHEBY", {"L": L, "K": RES_K, "use_bias": True, "activation": "relu", "device": str(dev)},
                                   activation="relu", use_bn=True, norm_type="layer_norm")
        x = torch.randn((N, M, d), generator=gen, device=dev)
        with torch.no_grad():
            block(x)
        native_ok = gnn_layers._ln_native_ok

        def new(a, training):
            return block(a, training=training)

        def parent(a, training):  # the same block with its norms on torch.nn.LayerNorm, as before the kernels
            gnn_layers._ln_native_ok = lambda mod, t: False
            try:
                return block(a, training=training)
            finally:
                gnn_layers._ln_native_ok = native_ok
        params = list(block.parameters())
    else:
        tables = None
        if kind == "sparse":
            nbr = grid_neighbour_table(size, dev)
            tables = (nbr, nbr)
        block = gnn_transformers.MultiHeadAttention(d_model=d, num_heads=heads, dense=kind == "dense").to(dev)
        with torch.no_grad():
            for p in block.parameters():
                if p.dim() == 1:
                    p.add_(0.1 * torch.randn(p.shape, generator=gen, device=dev))
        x = torch.randn((N, M, d), generator=gen, device=dev)

        def new(a, training):
            return block(a, tables=tables)

        def parent(a, training):
            t = block.layer_norm1(a)
            qkv = block.wqkv(t)
            if kind == "dense":
                att = gnn_transformers._DenseAttentionPacked.apply(qkv, heads)
            else:
                att = gnn_transformers._SparseAttentionPacked.apply(qkv, tables[0], tables[1], heads)
            att = t + att
            out = block.activation(block.dense(block.layer_norm2(att)))
            return out + att
        params = list(block.parameters())
    dy = torch.randn((N, M, d), generator=gen, device=dev)
    xg = x.clone().requires_grad_(True)

    def forward(f):
        def run():
            with torch.no_grad():
                return f(x, False)
        return run

    def step(f):
        def run():
            xg.grad = None
            for p in params:
                p.grad = None
            f(xg, True).backward(dy)
        return run

    return {"new": (forward(new), step(new)), "parent": (forward(parent), step(parent))}


def report(shape, level, p, warmup, reps, extra):
    a, b = p["new"][0](), p["parent"][0]()
    a, b = (a[0], b[0]) if isinstance(a, tuple) else (a, b)
    diff = float((a - b).abs().max() / b.abs().max())
    del a, b
    print(f"  ({level}) outputs of the two paths: max |difference| / max |z| = {diff:.2e}", flush=True)
    fwd = alternate({name: fns[0] for name, fns in p.items()}, warmup, reps)
    step = alternate({name: fns[1] for name, fns in p.items()}, warmup, reps)
    mem = {name: peak_memory(fns[1]) for name, fns in p.items()}
    for title, res in (("forward", fwd), ("forward + backward", step)):
        for name, (med, lo, hi) in res.items():
            print(f"  ({level}) {title:20s} {name:8s} {med:10.4f} ms   (min {lo:.4f}, max {hi:.4f}, {reps} calls)")
        print(f"  ({level}) {title:20s} parent / new = {res['parent'][0] / res['new'][0]:.3f}")
    print(f"  ({level}) peak memory of forward + backward above the resident tensors: new {mem['new'] / 2**20:.1f} MiB, "
          f"parent {mem['parent'] / 2**20:.1f} MiB")
    print(json.dumps({"shape": shape, "level": level, **extra, "output_difference": diff, "forward_ms": fwd, "forward_backward_ms": step,
                      "peak_bytes": mem}), flush=True)


def measure(shape, dev, warmup, reps, levels):
    kind, N, M, d = dims(shape)
    print(f"{shape}: {kind}, batch {N}, M {M}, d {d}; one pass over the map is {4 * N * M * d / 1e9:.3f} GB", flush=True)
    extra = {"kind": kind, "batch": N, "M": M, "d": d}
    if "a" in levels:
        p, with_res = level_a(shape, dev)
        report(shape, "a", p, warmup, reps, {**extra, "with_res": with_res})
        del p
        torch.cuda.empty_cache()
    if "b" in levels:
        p = level_b(shape, dev)
        report(shape, "b", p, warmup, reps, extra)
        del p
        torch.cuda.empty_cache()


def profile(shape, dev, steps=5):
    p, _ = level_a(shape, dev)
    for _ in range(steps):
        p["new"][1]()
    torch.cuda.synchronize()
    print(f"profile run: {steps} forward + backward calls of the kernels at {shape}")


def kernel_stats(directory, shape):
    kind, N, M, d = dims(shape)
    with_res = kind != "residual"
    map_bytes = 4 * N * M * d
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel_stats.csv under {directory}")
    out = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            for key, passes in PASSES.items():
                if key in r["Name"]:
                    reads, writes = passes[with_res]
                    avg_ms = float(r["AverageNs"]) / 1e6
                    out[key] = {"calls": int(r["Calls"]), "avg_ms": avg_ms, "passes": reads + writes,
                                "TB_per_s": (reads + writes) * map_bytes / (avg_ms * 1e-3) / 1e12}
            if "partials_merge_kernel" in r["Name"]:
                out["partials_merge_kernel"] = {"calls": int(r["Calls"]), "avg_ms": float(r["AverageNs"]) / 1e6}
    print(f"{shape}: one pass over the map is {map_bytes / 1e9:.3f} GB")
    for key, v in out.items():
        extra = f"{v['passes']} passes, {v['TB_per_s']:.2f} TB/s" if "passes" in v else "the fixed-order merge of the partials"
        print(f"  {key:22s} {v['calls']:4d} calls, {v['avg_ms']:9.4f} ms each   ({extra})")
    print(json.dumps({"shape": shape, "map_bytes": map_bytes, "kernels": out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="gt256,gt64,vit,res256")
    ap.add_argument("--levels", default="a,b")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile", metavar="SHAPE", default=None, choices=sorted(SHAPES))
    ap.add_argument("--kernel-stats", metavar="DIR", default=None)
    args = ap.parse_args()
    if args.kernel_stats:
        kernel_stats(args.kernel_stats, args.profile or "gt256")
        return
    _native.require_gpu()
    dev = torch.device("cuda", 0)
    if args.profile:
        profile(args.profile, dev)
        return
    for shape in args.shapes.split(","):
        measure(shape, dev, args.warmup, args.reps, args.levels.split(","))
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
