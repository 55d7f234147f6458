"""Independent restatement of the reference's dense attention and of ``Graph_ViT`` (helper, not collected by pytest).

The reference's algorithm (``gnn_transformers.scaled_dot_product_attention`` with ``mask=None``) written from its description:
the logits q_i . k_j / sqrt(depth) of every pair of rows and every head as one (N, heads, M, M) array, the softmax over j, the
product with v.  Once in numpy float64 for the forward checks (it also returns the logits and the log-sum-exp), once in torch in
whatever dtype the inputs have, so that float64 autograd supplies the reference gradients and a float32 run on the CPU the error
an fp32 implementation shows.  The whole ``Graph_ViT`` follows, from a dict of parameters named like the module's.
"""

import numpy as np
import torch

from attention_ref import _ACTS, _layer_norm


def attention_np(q, k, v, num_heads):
    """float64 numpy: q, k, v (N, M, d) -> out (N, M, d), logits (N, heads, M, M), lse (N, M, heads)."""
    q, k, v = (np.asarray(t, dtype=np.float64) for t in (q, k, v))
    N, M, d = q.shape
    D = d // num_heads
    q4, k4, v4 = (t.reshape(N, M, num_heads, D).transpose(0, 2, 1, 3) for t in (q, k, v))  # (N, heads, M, D)
    s = q4 @ k4.transpose(0, 1, 3, 2) / np.sqrt(D)
    mx = s.max(-1, keepdims=True)
    e = np.exp(s - mx)
    den = e.sum(-1, keepdims=True)
    out = (e / den) @ v4
    lse = (mx + np.log(den))[..., 0]  # (N, heads, M)
    return out.transpose(0, 2, 1, 3).reshape(N, M, d), s, lse.transpose(0, 2, 1)


def attention_torch(q, k, v, num_heads):
    """The same in torch, differentiable, in the dtype of q."""
    N, M, d = q.shape
    D = d // num_heads
    q4, k4, v4 = (t.reshape(N, M, num_heads, D).permute(0, 2, 1, 3) for t in (q, k, v))
    s = q4 @ k4.transpose(-1, -2) / float(np.sqrt(D))
    return (torch.softmax(s, dim=-1) @ v4).permute(0, 2, 1, 3).reshape(N, M, d)


def attention_grads64(q, k, v, num_heads, gout):
    """out, dq, dk, dv by float64 autograd of ``attention_torch`` (numpy in, numpy out)."""
    t = [torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True) for a in (q, k, v)]
    out = attention_torch(t[0], t[1], t[2], num_heads)
    out.backward(torch.as_tensor(np.asarray(gout, dtype=np.float64)))
    return (out.detach().numpy(),) + tuple(a.grad.numpy() for a in t)


def graph_vit(x, params, p, num_heads, n_layers=1, positional_encoding=True, layer_norm=True, activation="relu"):
    """The whole layer from ``params`` (name -> tensor, the names of ``Graph_ViT.named_parameters()``; ``embed.weight`` is the
    Conv1d's (d, Fin, 4^p), Linear weights are (out, in)), in the dtype of x: the strided convolution written as a sum over the
    4^p positions of a patch, the position embedding, then per block norm -> q | k | v -> dense attention -> + normed input ->
    norm -> dense -> activation -> + residual."""
    act = _ACTS[activation]
    g = 4 ** p
    N, M, Fin = x.shape
    w = params["embed.weight"]
    patches = x.reshape(N, M // g, g, Fin)
    x = torch.einsum("nmif,ofi->nmo", patches, w) + params["embed.bias"]
    if positional_encoding:
        x = x + params["pos_encoder.pos_embedding"]
    d = x.shape[-1]
    for i in range(n_layers):
        pre = f"mha_layers.{i}."
        if layer_norm:
            x = _layer_norm(x, params[pre + "layer_norm1.weight"], params[pre + "layer_norm1.bias"])
        qkv = x @ params[pre + "wqkv.weight"].T + params[pre + "wqkv.bias"]
        att = x + attention_torch(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], num_heads)
        y = att
        if layer_norm:
            y = _layer_norm(att, params[pre + "layer_norm2.weight"], params[pre + "layer_norm2.bias"])
        x = act(y @ params[pre + "dense.weight"].T + params[pre + "dense.bias"]) + att
    return x


def graph_vit_grads(x, params, gout, dtype, **kw):
    """(out, {name: grad}) of sum(out * gout) on the CPU in ``dtype``."""
    p = {n: torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for n, a in params.items()}
    out = graph_vit(torch.tensor(np.asarray(x), dtype=dtype), p, **kw)
    out.backward(torch.tensor(np.asarray(gout), dtype=dtype))
    return out.detach().numpy(), {n: a.grad.numpy() for n, a in p.items()}
