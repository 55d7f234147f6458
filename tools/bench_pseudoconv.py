#!/usr/bin/env python3
"""Time the pseudo-convolutions on the patch GEMM against the torch composition the parent commit ran, on one GPU.

    python tools/bench_pseudoconv.py [--shapes mid,wide,p2,first] [--precisions auto,fp32,bf16x3] [--reps 20] [--warmup 3]

Per shape, layer (``HealpyPseudoConv`` "down", ``HealpyPseudoConv_Transpose`` "up") and arithmetic: the layer as it is now against
the parent's composition written out here on the same weights -- ``torch.addmm`` on the free reshape for the reduction, ``@`` and a
bias add over the 4^p times larger map for the expansion, then the ``torch`` activation, gradients from autograd.  Both paths in
this process, taking turns after a warm-up, each call between two device events; medians with the smallest and largest beside
them (the spread of a path against itself).  Forward under ``torch.no_grad()``, and forward + backward (gradients of the map, the
weights and the bias); peak memory of one forward + backward beyond what is allocated before it.  Shapes (nside of the finer map):
  mid      nside 512, batch 8, 64 -> 64, p = 1, elu: the middle of a U-Net / autoencoder
  wide     nside 1024, batch 4, 16 -> 32, p = 1, relu
  p2       nside 256, batch 8, 32 -> 32, p = 2, no activation
  first    nside 512, batch 8, 1 -> 16, p = 1, no activation: a first layer
Under "auto" the layers run the kernel where Kd <= 64 and C <= 256 and keep the composition beyond (their shape rule, set from
these figures): there the "auto" rows time the composition against itself, and the rows of the named arithmetics show the kernel.
``share`` is the achieved share of 6.3e12 B/s for the least traffic of the forward, 4 (R Kd + R C) bytes.
Sets no threshold.  Prints the figures and one JSON line per case.  Needs a GPU: there is no figure without one.
"""

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "deepsphere-cosmo-tf2_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from deepsphere import healpy_layers  # noqa: E402

# nside of the finer map, batch, Fin, Fout, p, activation
SHAPES = {"mid": (512, 8, 64, 64, 1, "elu"), "wide": (1024, 4, 16, 32, 1, "relu"), "p2": (256, 8, 32, 32, 2, None),
          "first": (512, 8, 1, 16, 1, None)}
HBM_RATE = 6.3e12  # achievable bytes/s of an MI355X
ACT = {None: None, "elu": torch.nn.functional.elu, "relu": torch.relu}


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


def parent_forward(layer, x, up):
    """The composition of the parent commit on the layer's own parameters."""
    N, M, Fin = x.shape
    g, Fout, f = layer.filter_size, layer.Fout, layer.filter
    if up:
        w2 = f.weight.permute(0, 2, 1).reshape(Fin, g * Fout)
        y = (x.reshape(N * M, Fin) @ w2).reshape(N, M * g, Fout) + f.bias
    else:
        w2 = f.weight.permute(2, 1, 0).reshape(g * Fin, Fout)
        y = torch.addmm(f.bias, x.reshape(N * (M // g), g * Fin), w2).reshape(N, M // g, Fout)
    return y if layer.activation is None else layer.activation(y)


def bench(shape, up, precision, warmup, reps, dev):
    nside, N, Fin, Fout, p, act = SHAPES[shape]
    g = 4 ** p
    M_fine = 12 * nside * nside
    M_in = M_fine // g if up else M_fine
    cls = healpy_layers.HealpyPseudoConv_Transpose if up else healpy_layers.HealpyPseudoConv
    torch.manual_seed(0)
    layer = cls(p, Fout, activation=act, precision=precision, bias_initializer=lambda b: torch.nn.init.normal_(b, std=0.3))
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((N, M_in, Fin), generator=gen, device=dev)
    layer(x[:1])  # builds the filter
    R, Kd, C = (N * M_in, Fin, g * Fout) if up else (N * M_in // g, g * Fin, Fout)
    dy = torch.randn((N, M_in * g if up else M_in // g, Fout), generator=gen, device=dev)
    xg = x.clone().requires_grad_(True)

    def step(forward):
        def run():
            xg.grad = None
            layer.zero_grad(set_to_none=True)
            forward(xg).backward(dy)
        return run

    def nograd(forward):
        def run():
            with torch.no_grad():
                forward(x)
        return run

    new, parent = layer, lambda t: parent_forward(layer, t, up)
    with torch.no_grad():
        diff = float((new(x) - parent(x)).abs().max() / parent(x).abs().max())
    fwd = alternate({"new": nograd(new), "parent": nograd(parent)}, warmup, reps)
    both = alternate({"new": step(new), "parent": step(parent)}, warmup, reps)
    mem = {name: peak_memory(step(f)) for name, f in (("new", new), ("parent", parent))}
    traffic = 4.0 * (R * Kd + R * C)
    out = {"shape": shape, "layer": "up" if up else "down", "precision": precision, "R": R, "Kd": Kd, "C": C, "activation": act,
           "max_rel_diff_to_parent": diff}
    for level, res in (("forward", fwd), ("forward_backward", both)):
        for name, (med, lo, hi) in res.items():
            out[f"{level}_{name}_ms"] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4)}
        out[f"{level}_speedup"] = round(res["parent"][0] / res["new"][0], 3)
        out[f"{level}_parent_spread"] = round((res["parent"][2] - res["parent"][1]) / res["parent"][0], 4)
    out["forward_hbm_share"] = {name: round(traffic / (fwd[name][0] * 1e-3) / HBM_RATE, 3) for name in fwd}
    out["peak_mib"] = {name: round(v / 2**20, 1) for name, v in mem.items()}
    print(f"{shape:5s} {out['layer']:4s} {precision:6s} R {R} Kd {Kd} C {C}: forward {fwd['new'][0]:.3f} ms vs {fwd['parent'][0]:.3f} "
          f"(x{out['forward_speedup']}, HBM share {out['forward_hbm_share']['new']:.2f} vs {out['forward_hbm_share']['parent']:.2f}); "
          f"forward + backward {both['new'][0]:.3f} ms vs {both['parent'][0]:.3f} (x{out['forward_backward_speedup']}); "
          f"peak {out['peak_mib']['new']} vs {out['peak_mib']['parent']} MiB; |new - parent| {diff:.1e}")
    print(json.dumps(out))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--precisions", default="auto,fp32,bf16x3")
    ap.add_argument("--layers", default="down,up")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pseudoconv needs a GPU")
    dev = torch.device("cuda:0")
    for shape in args.shapes.split(","):
        for which in args.layers.split(","):
            for precision in args.precisions.split(","):
                bench(shape, which == "up", precision, args.warmup, args.reps, dev)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
