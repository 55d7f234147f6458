"""Restatement of the dense attention WITH the reference's mask argument, and of ``Graph_ViT`` with it (helper, not collected).

Written from the description of the semantics, not from any implementation:

    s_ij = q_i . k_j / sqrt(depth)      computed in float64, rounded to float32
    x_ij = s_ij + float32(mask_ij) * float32(-1e9)      product and sum in float32
    P = softmax_j(x),  out = P v,  statistic pair (m, log l) = (max_j x, log sum_j exp(x - m))      float64 from here on

The mask broadcasts against the (N, heads, M, M) logits.  It is an add: a fractional mask is a soft bias.  With every key of a
row masked, x is exactly -1e9 wherever |s| < 32 (the ulp of float32 at 1e9 is 64), the row's softmax is uniform and its output the
mean of v; the helper asserts max |s| < 16 on its inputs so that the argument holds with room.

Gradients are analytic from P:  dV = P^T dO,  dP = dO V^T,  dS = P o (dP - rowsum(dO o O)),  dQ = scale dS K,  dK = scale dS^T Q.

``split_attention`` is the mask-aware emulation of the two bf16 split arithmetics, built from ``split`` / ``split_matmul`` of
tests/dense_attention_split_ref.py (operand rounding only, partial products summed in float64); the mask enters after the first
product, on the float32 logit, and is never split.  ``graph_vit`` is the whole layer in torch, in the dtype of its input.
"""

import numpy as np
import torch

from attention_ref import _ACTS, _layer_norm
from dense_attention_split_ref import TERMS, split_matmul

S_LIMIT = 16.0
WEIGHT = np.float32(-1e9)


def _heads_first(t, num_heads):
    N, M, d = t.shape
    return t.reshape(N, M, num_heads, d // num_heads).transpose(0, 2, 1, 3)  # (N, heads, M, D)


def _rows_first(t):
    N, H, M, D = t.shape
    return t.transpose(0, 2, 1, 3).reshape(N, M, H * D)


def _t(a):
    return a.transpose(0, 1, 3, 2)


def masked_logits(s64, mask):
    """float64 logits (N, heads, M, M) -> x in float64 holding float32 values: round, add float32(mask) * float32(-1e9) in float32."""
    assert np.abs(s64).max() < S_LIMIT, "the absorption argument of the fully masked row needs |s| < 32; the helper asks 16"
    s32 = s64.astype(np.float32)
    bias = np.asarray(mask).astype(np.float32) * WEIGHT  # float32 product
    bias = np.broadcast_to(bias.reshape((1,) * (4 - bias.ndim) + bias.shape), s32.shape)
    return (s32 + bias).astype(np.float64)  # float32 sum


def _softmax_stats(x):
    m = x.max(-1, keepdims=True)
    e = np.exp(x - m)
    l = e.sum(-1, keepdims=True)
    return e / l, m, np.log(l)


def _pack_stat(m, logl):
    """(N, heads, M, 1) x 2 -> (N, M, heads, 2)"""
    return np.stack([m[..., 0].transpose(0, 2, 1), logl[..., 0].transpose(0, 2, 1)], axis=-1)


def attention(q, k, v, num_heads, mask, gout=None):
    """float64 reference: -> (out (N, M, d), stat (N, M, heads, 2)), with ``gout`` also dq, dk, dv."""
    q4, k4, v4 = (_heads_first(np.asarray(t, dtype=np.float64), num_heads) for t in (q, k, v))
    scale = 1.0 / np.sqrt(q4.shape[-1])
    x = masked_logits(q4 @ _t(k4) * scale, mask)
    P, m, logl = _softmax_stats(x)
    out4 = P @ v4
    res = (_rows_first(out4), _pack_stat(m, logl))
    if gout is None:
        return res
    g4 = _heads_first(np.asarray(gout, dtype=np.float64), num_heads)
    dv4 = _t(P) @ g4
    dp = g4 @ _t(v4)
    ds = P * (dp - (g4 * out4).sum(-1, keepdims=True))
    return res + (_rows_first(ds @ k4 * scale), _rows_first(_t(ds) @ q4 * scale), _rows_first(dv4))


def split_attention(q, k, v, num_heads, precision, mask, gout=None):
    """The same through the emulated split arithmetic ``precision``: every matrix product by ``split_matmul``, the mask added to
    the float32-rounded logit.  -> (out, stat[, dq, dk, dv]) in float64."""
    terms = TERMS[precision]
    q4, k4, v4 = (_heads_first(np.asarray(t, dtype=np.float32), num_heads) for t in (q, k, v))
    scale = 1.0 / np.sqrt(q4.shape[-1])
    x = masked_logits(split_matmul(q4, _t(k4), terms) * scale, mask)
    m = x.max(-1, keepdims=True)
    e = np.exp(x - m)
    l = e.sum(-1, keepdims=True)
    out4 = split_matmul(e.astype(np.float32), v4, terms) / l
    res = (_rows_first(out4), _pack_stat(m, np.log(l)))
    if gout is None:
        return res
    g4 = _heads_first(np.asarray(gout, dtype=np.float32), num_heads)
    P = e / l
    dp = split_matmul(g4, _t(v4), terms)
    delta = (g4.astype(np.float64) * out4).sum(-1, keepdims=True)
    ds = (P * (dp - delta)).astype(np.float32)
    return res + (_rows_first(split_matmul(ds, k4, terms) * scale), _rows_first(split_matmul(_t(ds), q4, terms) * scale),
                  _rows_first(split_matmul(_t(P.astype(np.float32)), g4, terms)))


def attention_torch(q, k, v, num_heads, mask):
    """Differentiable, in the dtype of q; the mask's addend is formed in float32 as above, then cast."""
    N, M, d = q.shape
    D = d // num_heads
    q4, k4, v4 = (t.reshape(N, M, num_heads, D).permute(0, 2, 1, 3) for t in (q, k, v))
    s = q4 @ k4.transpose(-1, -2) / float(np.sqrt(D))
    bias = torch.as_tensor(np.asarray(mask).astype(np.float32) * WEIGHT).to(s.dtype)
    return (torch.softmax(s + bias, dim=-1) @ v4).permute(0, 2, 1, 3).reshape(N, M, d)


def mha_block(x, params, pre, num_heads, mask, layer_norm=True, activation="relu"):
    """One block: norm -> q | k | v -> masked dense attention -> + normed input -> norm -> dense -> activation -> + residual."""
    act = _ACTS[activation]
    d = x.shape[-1]
    if layer_norm:
        x = _layer_norm(x, params[pre + "layer_norm1.weight"], params[pre + "layer_norm1.bias"])
    qkv = x @ params[pre + "wqkv.weight"].T + params[pre + "wqkv.bias"]
    att = x + attention_torch(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], num_heads, mask)
    y = att
    if layer_norm:
        y = _layer_norm(att, params[pre + "layer_norm2.weight"], params[pre + "layer_norm2.bias"])
    return act(y @ params[pre + "dense.weight"].T + params[pre + "dense.bias"]) + att


def graph_vit(x, params, p, num_heads, mask, n_layers=1, positional_encoding=True, layer_norm=True, activation="relu"):
    """The whole layer from ``params`` (the names of ``Graph_ViT.named_parameters()``), the same mask in every block."""
    g = 4 ** p
    N, M, Fin = x.shape
    x = torch.einsum("nmif,ofi->nmo", x.reshape(N, M // g, g, Fin), params["embed.weight"]) + params["embed.bias"]
    if positional_encoding:
        x = x + params["pos_encoder.pos_embedding"]
    for i in range(n_layers):
        x = mha_block(x, params, f"mha_layers.{i}.", num_heads, mask, layer_norm, activation)
    return x


def grads(fn, x, params, gout, dtype):
    """(out, dx, {name: grad}) of sum(fn(x, params) * gout) on the CPU in ``dtype``."""
    p = {n: torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for n, a in params.items()}
    xt = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    out = fn(xt, p)
    out.backward(torch.tensor(np.asarray(gout), dtype=dtype))
    return out.detach().numpy(), xt.grad.numpy(), {n: a.grad.numpy() for n, a in p.items() if a.grad is not None}
