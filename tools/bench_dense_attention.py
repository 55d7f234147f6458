#!/usr/bin/env python3
"""Time the dense-attention kernels against the same attention written the reference's way in torch, on one GPU.

    python tools/bench_dense_attention.py [--tokens 3072] [--batch 8] [--heads 4] [--depth 32] [--reps 30] [--warmup 5]
                                          [--mask none|key|pair]

(a) the kernel forward, (b) kernel forward + backward, (c) the reference formulation on the same device: the (N, heads, M, M)
logits materialised by a matmul, softmax, a second matmul -- forward and forward + backward through autograd.  Both sides run in
this process, alternating, after a warm-up; times are medians of device-event timings of single calls.  The default shape is the
3,072 tokens of nside 64 at p = 2 (or nside 32 at p = 1), 4 heads of 32 channels, 8 maps.  FLOPs: the algorithm needs two
products of 2 N heads M^2 depth each forward (4 N heads M^2 depth), and 2.5 times that backward (five products); the kernels'
backward recomputes the logits in both passes (seven products).  The rate is the algorithmic FLOPs over the time, against the
157 TFLOP/s of the fp32 MFMA (64 FLOP / clk / SIMD x 4 SIMDs x 256 CUs x 2.4 GHz).  Peak memory: torch.cuda.max_memory_allocated
over one call of each side, above what q, k, v and the upstream gradient occupy.  The two bf16 split arithmetics of the kernels
(``precision`` PREC_BF16X6, PREC_BF16X3; depth 32 and 64) are further cases of the same alternating loop, ``bf16x6_*`` and
``bf16x3_*``, with their own agreement figures and their time against the fp32 kernels' (``kernel_*``, the baseline).  Prints
the figures and one JSON line.  Needs a GPU: there is no CPU fallback and no figure without one.

``--mask key`` (a per-map key mask (N, 1, 1, M)) or ``--mask pair`` (a shared pair mask (M, M)), random 0 / 1 with 30 % ones:
every kernel case above then runs the masked entry points, the materialised side adds ``mask * -1e9`` to its logits the
reference's way, and the unmasked kernels join the same alternating loop as ``nomask_*`` (fp32) and ``nomask_bf16x?_*`` -- the
price of the mask is the ratio against them.  ``--mask none`` (default) is the tool as it was.
"""

import argparse
import functools
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

from deepsphere import _native  # noqa: E402

FP32_MFMA_PEAK = 64 * 4 * 256 * 2.4e9  # FLOP / s


def materialised_attention(q, k, v, heads, mask=None):
    """The reference's algorithm on (N, M, d) tensors: split_heads' transposes, matmul, scale, [+ mask * -1e9,] softmax, matmul,
    transpose back."""
    N, M, d = q.shape
    D = d // heads
    q4, k4, v4 = (t.reshape(N, M, heads, D).permute(0, 2, 1, 3) for t in (q, k, v))
    logits = torch.matmul(q4, k4.transpose(-1, -2)) / float(np.sqrt(D))
    if mask is not None:
        logits = logits + mask * -1e9
    weights = torch.softmax(logits, dim=-1)
    return torch.matmul(weights, v4).permute(0, 2, 1, 3).reshape(N, M, d)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def peak_bytes(fn):
    """Peak of the allocator over one call, above what was allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    r = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del r
    return int(peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=3072)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--depth", type=int, default=32)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-baseline", action="store_true", help="time the kernels only (token counts whose logits do not fit)")
    ap.add_argument("--mask", choices=("none", "key", "pair"), default="none",
                    help="run the masked entry points: a per-map key mask (N, 1, 1, M) or a shared pair mask (M, M)")
    args = ap.parse_args()
    _native.require_gpu()
    dev = torch.device("cuda", 0)
    M, heads, d, N = args.tokens, args.heads, args.heads * args.depth, args.batch
    gen = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn((N, M, 3 * d), generator=gen, device=dev)  # the layout the layer hands the kernel: three strided views
    g = torch.randn((N, M, d), generator=gen, device=dev)
    q, k, v = qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:]
    mask, mkw = None, {}
    if args.mask != "none":
        shape = (N, 1, 1, M) if args.mask == "key" else (M, M)
        mask = (torch.rand(shape, generator=gen, device=dev) < 0.3).to(torch.float32)
        mask[..., 0] = 0.0  # (every row keeps a key)
        mkw = {"mask": mask}

    def kernel_fwd(precision=_native.PREC_FP32, **kw):
        return _native.dense_attention(q, k, v, heads, precision=precision, **kw)

    def kernel_fwd_bwd(precision=_native.PREC_FP32, **kw):
        out, lse = _native.dense_attention(q, k, v, heads, precision=precision, **kw)
        return _native.dense_attention_backward(q, k, v, out, lse, g, heads, precision=precision, **kw)

    def torch_fwd():
        with torch.no_grad():
            return materialised_attention(q, k, v, heads, mask)

    def torch_fwd_bwd():
        t = [a.detach().requires_grad_(True) for a in (q, k, v)]
        materialised_attention(t[0], t[1], t[2], heads, mask).backward(g)
        return [a.grad for a in t]

    cases = {"kernel_fwd": functools.partial(kernel_fwd, **mkw), "kernel_fwd_bwd": functools.partial(kernel_fwd_bwd, **mkw)}
    splits = {"bf16x6": _native.PREC_BF16X6, "bf16x3": _native.PREC_BF16X3} if args.depth in (32, 64) else {}
    for name, code in splits.items():
        cases[name + "_fwd"] = functools.partial(kernel_fwd, code, **mkw)
        cases[name + "_fwd_bwd"] = functools.partial(kernel_fwd_bwd, code, **mkw)
    if mask is not None:  # the unmasked kernels in the same loop: what the mask costs
        for prefix, code in [("nomask", _native.PREC_FP32)] + [("nomask_" + n, c) for n, c in splits.items()]:
            cases[prefix + "_fwd"] = functools.partial(kernel_fwd, code)
            cases[prefix + "_fwd_bwd"] = functools.partial(kernel_fwd_bwd, code)
    agree = {}
    if not args.skip_baseline:
        cases.update({"torch_fwd": torch_fwd, "torch_fwd_bwd": torch_fwd_bwd})
        # same numbers first (faster and different is not faster)
        out_t, gt = torch_fwd(), torch_fwd_bwd()
        for prefix, code in [("", _native.PREC_FP32)] + [(n + "_", c) for n, c in splits.items()]:
            out_k, gk = kernel_fwd(code, **mkw)[0], kernel_fwd_bwd(code, **mkw)
            agree[prefix + "out"] = float((out_k - out_t).abs().max() / out_t.abs().max())
            for name, a, b in zip(("dq", "dk", "dv"), gk, gt):
                agree[prefix + name] = float((a - b).abs().max() / b.abs().max())
        del out_k, out_t, gk, gt
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
    peaks = {name: peak_bytes(fn) for name, fn in cases.items()}
    flops_fwd = 4.0 * N * heads * M * M * args.depth
    flops = {name: 3.5 * flops_fwd if name.endswith("_fwd_bwd") else flops_fwd for name in cases}
    print(f"{M} tokens, batch {N}, {heads} heads x {args.depth}; logits of one call: {N * heads * M * M * 4 / 2**20:.0f} MiB; "
          f"q: {N * M * d * 4 / 2**20:.1f} MiB; device: {torch.cuda.get_device_name(0)}")
    if agree:
        print("agreement kernel vs materialised (max rel): " + ", ".join(f"{n} {e:.1e}" for n, e in agree.items()))
    for name in cases:
        rate = flops[name] / (ms[name] * 1e-3)
        print(f"{name:16s} {ms[name]:9.3f} ms   (min {spread[name][0]:.3f}, max {spread[name][1]:.3f}, {args.reps} calls)   "
              f"{rate / 1e12:6.1f} TFLOP/s algorithmic = {rate / FP32_MFMA_PEAK:.2f} of the fp32 MFMA peak   "
              f"peak memory {peaks[name] / 2**20:9.1f} MiB")
    result = {"tokens": M, "batch": N, "heads": heads, "depth": args.depth, "ms": ms, "min_max_ms": spread, "peak_bytes": peaks,
              "flops_fwd": flops_fwd, "agreement": agree}
    if mask is not None:
        result["mask"] = args.mask
        for prefix, base in [("kernel", "nomask")] + [(n, "nomask_" + n) for n in splits]:
            for tail in ("_fwd", "_fwd_bwd"):
                result[f"masked_over_unmasked_{prefix}{tail}"] = ms[prefix + tail] / ms[base + tail]
            print(f"{args.mask} mask / no mask, {prefix}: forward {result[f'masked_over_unmasked_{prefix}_fwd']:.2f} x, "
                  f"forward + backward {result[f'masked_over_unmasked_{prefix}_fwd_bwd']:.2f} x")
    for name in splits:
        result[f"fp32_over_{name}_fwd"] = ms["kernel_fwd"] / ms[name + "_fwd"]
        result[f"fp32_over_{name}_fwd_bwd"] = ms["kernel_fwd_bwd"] / ms[name + "_fwd_bwd"]
        print(f"fp32 kernels / {name}: forward {result[f'fp32_over_{name}_fwd']:.2f} x, "
              f"forward + backward {result[f'fp32_over_{name}_fwd_bwd']:.2f} x")
    if not args.skip_baseline:
        result["ratio_fwd"] = ms["torch_fwd"] / ms["kernel_fwd"]
        result["ratio_fwd_bwd"] = ms["torch_fwd_bwd"] / ms["kernel_fwd_bwd"]
        print(f"materialised / kernel: forward {result['ratio_fwd']:.2f} x, forward + backward {result['ratio_fwd_bwd']:.2f} x; "
              f"peak memory forward {peaks['torch_fwd'] / max(peaks['kernel_fwd'], 1):.0f} x, "
              f"forward + backward {peaks['torch_fwd_bwd'] / max(peaks['kernel_fwd_bwd'], 1):.0f} x")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
