#!/usr/bin/env python3
"""Time the neighbour-attention kernels against the same attention written the reference's way in torch, on one GPU.

    python tools/bench_attention.py [--nside 256] [--batch 2] [--heads 4] [--depth 16] [--neighbors 8] [--reps 30] [--warmup 5]

(a) the kernel forward, (b) kernel forward + backward, (c) the reference formulation on the same device: q, k, v looked up per
edge (index_select), exp, segment sums (index_add_), divide -- forward and forward + backward through autograd.  Both sides run in
this process, alternating, after a warm-up; times are medians of device-event timings of single calls.  Bytes: the algorithm
needs q, k, v in and out out once, 4 N M d 4 bytes; the kernel REQUESTS q + out + (k + v) per neighbour + the table (most
neighbour rows are served by L2).  The rate is the algorithmic bytes over the time, against the 6.3 TB/s an MI355X reaches from
HBM.  Prints the figures and one JSON line.  Needs a GPU: there is no CPU fallback and no figure without one.
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

from deepsphere import _native, gnn_transformers, healpix  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes / s


def edge_list_attention(q, k, v, rows, cols, heads):
    """The reference's algorithm on (N, M, d) tensors: the pixel axis first (its transposes), per-edge lookups, exp of the raw
    logits, two segment sums, the quotient."""
    N, M, d = q.shape
    D = d // heads
    qs, ks, vs = (t.reshape(N, M, heads, D).permute(1, 0, 2, 3) for t in (q, k, v))
    q_part, k_part, v_part = qs.index_select(0, rows), ks.index_select(0, cols), vs.index_select(0, cols)
    e = torch.exp((q_part * k_part).sum(-1, keepdim=True) / float(np.sqrt(D)))
    den = torch.zeros((M, N, heads, 1), dtype=q.dtype, device=q.device).index_add_(0, rows, e)
    num = torch.zeros((M, N, heads, D), dtype=q.dtype, device=q.device).index_add_(0, rows, v_part * e)
    return (num / den).permute(1, 0, 2, 3).reshape(N, M, d)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nside", type=int, default=256)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--depth", type=int, default=16)
    ap.add_argument("--neighbors", type=int, default=8)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    _native.require_gpu()
    dev = torch.device("cuda", 0)
    A = healpix.healpix_graph(args.nside, n_neighbors=args.neighbors)
    M, heads, d, N = A.shape[0], args.heads, args.heads * args.depth, args.batch
    nbr, nbrT = gnn_transformers.neighbour_tables(A)
    same = nbr is nbrT
    nbr = nbr.to(dev)
    nbrT = nbr if same else nbrT.to(dev)
    r, c = A.nonzero()
    order = np.lexsort((c, r))
    rows, cols = torch.as_tensor(r[order].astype(np.int64), device=dev), torch.as_tensor(c[order].astype(np.int64), device=dev)
    E = int(rows.numel())
    gen = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn((N, M, 3 * d), generator=gen, device=dev)  # the layout the layer hands the kernel: three strided views
    g = torch.randn((N, M, d), generator=gen, device=dev)
    q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]

    def kernel_fwd():
        return _native.nbr_attention(q, k, v, nbr, heads)

    def kernel_fwd_bwd():
        out, lse = _native.nbr_attention(q, k, v, nbr, heads)
        return _native.nbr_attention_backward(q, k, v, out, lse, g, nbr, nbrT, heads)

    def torch_fwd():
        with torch.no_grad():
            return edge_list_attention(q, k, v, rows, cols, heads)

    def torch_fwd_bwd():
        t = [a.detach().requires_grad_(True) for a in (q, k, v)]
        edge_list_attention(t[0], t[1], t[2], rows, cols, heads).backward(g)
        return [a.grad for a in t]

    # same numbers first (faster and different is not faster)
    out_k, out_t = kernel_fwd()[0], torch_fwd()
    gk, gt = kernel_fwd_bwd(), torch_fwd_bwd()
    agree = {"out": float((out_k - out_t).abs().max() / out_t.abs().max())}
    for name, a, b in zip(("dq", "dk", "dv"), gk, gt):
        agree[name] = float((a - b).abs().max() / b.abs().max())
    del out_k, out_t, gk, gt
    cases = {"kernel_fwd": kernel_fwd, "torch_fwd": torch_fwd, "kernel_fwd_bwd": kernel_fwd_bwd, "torch_fwd_bwd": torch_fwd_bwd}
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
    alg = 4 * N * M * d * 4
    requested = N * (M * 2 * d * 4 + E * 2 * d * 4 + M * heads * 4) + N * M * nbr.shape[1] * 4
    rate = alg / (ms["kernel_fwd"] * 1e-3)
    print(f"nside {args.nside}: M {M}, {E} edges (width {nbr.shape[1]}), batch {N}, {heads} heads x {args.depth}")
    print(f"agreement kernel vs edge list (max rel): " + ", ".join(f"{n} {e:.1e}" for n, e in agree.items()))
    for name in cases:
        print(f"{name:16s} {ms[name]:9.3f} ms   (min {spread[name][0]:.3f}, max {spread[name][1]:.3f}, {args.reps} calls)")
    print(f"forward: algorithmic {alg / 1e9:.3f} GB, requested {requested / 1e9:.3f} GB ({requested / alg:.2f} x); "
          f"{rate / 1e12:.2f} TB/s algorithmic = {rate / HBM_ACHIEVABLE:.2f} of {HBM_ACHIEVABLE / 1e12:.1f} TB/s")
    print(f"edge list / kernel: forward {ms['torch_fwd'] / ms['kernel_fwd']:.1f} x, "
          f"forward + backward {ms['torch_fwd_bwd'] / ms['kernel_fwd_bwd']:.1f} x")
    print(json.dumps({"nside": args.nside, "M": M, "edges": E, "batch": N, "heads": heads, "depth": args.depth, "ms": ms,
                      "algorithmic_bytes": alg, "requested_bytes": requested, "hbm_fraction_fwd": rate / HBM_ACHIEVABLE,
                      "ratio_fwd": ms["torch_fwd"] / ms["kernel_fwd"],
                      "ratio_fwd_bwd": ms["torch_fwd_bwd"] / ms["kernel_fwd_bwd"], "agreement": agree}))


if __name__ == "__main__":
    main()
