"""Independent restatement of the reference's graph attention (helper, not collected by pytest).

The reference's algorithm (``gnn_transformers.scaled_dot_product_sparse_attention``) written from its description, per EDGE:
the positions ``A.nonzero()`` reports are the edges (i, j); per edge the product q_i . k_j / sqrt(depth) of every head, ``exp`` of
it, segment sums over the edges of a row of exp and of exp * v_j, and the quotient of the two.  Once in numpy float64
(``np.add.at``) for the forward checks, once in torch (``index_select`` / ``index_add_``) in whatever dtype the inputs have, so that
float64 autograd supplies the reference gradients and a float32 run on the CPU the error an fp32 implementation shows.  Rows
without an edge give 0 (the quotient is taken over 1 there; the reference has 0 / 0).  The whole ``Graph_Transformer`` follows,
from a dict of parameters named like the module's.
"""

import numpy as np
import torch
from scipy import sparse


def edges(A):
    """(rows, cols) of the edges: the positions numpy / scipy ``nonzero`` reports, stored zeros excluded."""
    rows, cols = sparse.csr_matrix(A).nonzero()
    return np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)


def attention_np(q, k, v, rows, cols, num_heads):
    """float64 numpy: q, k, v (N, M, d) -> (N, M, d)."""
    q, k, v = (np.asarray(t, dtype=np.float64) for t in (q, k, v))
    N, M, d = q.shape
    D = d // num_heads
    q4, k4, v4 = (t.reshape(N, M, num_heads, D) for t in (q, k, v))
    s = (q4[:, rows] * k4[:, cols]).sum(-1) / np.sqrt(D)  # (N, E, heads)
    e = np.exp(s)
    den = np.zeros((N, M, num_heads))
    num = np.zeros((N, M, num_heads, D))
    np.add.at(den, (slice(None), rows), e)
    np.add.at(num, (slice(None), rows), e[..., None] * v4[:, cols])
    out = num / np.where(den > 0, den, 1.0)[..., None]
    return out.reshape(N, M, d), s


def attention_torch(q, k, v, rows, cols, num_heads):
    """The same in torch, differentiable, in the dtype of q."""
    N, M, d = q.shape
    D = d // num_heads
    rows_t = torch.as_tensor(rows, dtype=torch.int64, device=q.device)
    cols_t = torch.as_tensor(cols, dtype=torch.int64, device=q.device)
    q4, k4, v4 = (t.reshape(N, M, num_heads, D) for t in (q, k, v))
    s = (q4.index_select(1, rows_t) * k4.index_select(1, cols_t)).sum(-1) / float(np.sqrt(D))
    e = torch.exp(s)
    den = torch.zeros((N, M, num_heads), dtype=q.dtype, device=q.device).index_add_(1, rows_t, e)
    num = torch.zeros((N, M, num_heads, D), dtype=q.dtype, device=q.device).index_add_(
        1, rows_t, e.unsqueeze(-1) * v4.index_select(1, cols_t))
    out = num / torch.where(den > 0, den, torch.ones_like(den)).unsqueeze(-1)
    return out.reshape(N, M, d)


def attention_grads64(q, k, v, rows, cols, num_heads, gout):
    """out, dq, dk, dv by float64 autograd of ``attention_torch`` (numpy in, numpy out)."""
    t = [torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True) for a in (q, k, v)]
    out = attention_torch(t[0], t[1], t[2], rows, cols, num_heads)
    out.backward(torch.as_tensor(np.asarray(gout, dtype=np.float64)))
    return (out.detach().numpy(),) + tuple(a.grad.numpy() for a in t)


def _layer_norm(x, gain, shift, eps=1e-3):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gain + shift


_ACTS = {"relu": torch.relu, "elu": torch.nn.functional.elu, "tanh": torch.tanh, "sigmoid": torch.sigmoid, None: lambda x: x}


def graph_transformer(x, params, rows, cols, num_heads, n_layers=1, positional_encoding=True, layer_norm=True,
                      activation="relu"):
    """The whole layer from ``params`` (name -> tensor, the names of ``Graph_Transformer.named_parameters()``; Linear weights
    are (out, in)), in the dtype of x: embedding, position embedding, then per block norm -> q | k | v -> attention -> + normed
    input -> norm -> dense -> activation -> + residual."""
    act = _ACTS[activation]
    x = x @ params["embed.weight"].T + params["embed.bias"]
    if positional_encoding:
        x = x + params["pos_encoder.pos_embedding"]
    d = x.shape[-1]
    for i in range(n_layers):
        p = f"mha_layers.{i}."
        if layer_norm:
            x = _layer_norm(x, params[p + "layer_norm1.weight"], params[p + "layer_norm1.bias"])
        qkv = x @ params[p + "wqkv.weight"].T + params[p + "wqkv.bias"]
        att = x + attention_torch(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:], rows, cols, num_heads)
        y = att
        if layer_norm:
            y = _layer_norm(att, params[p + "layer_norm2.weight"], params[p + "layer_norm2.bias"])
        x = act(y @ params[p + "dense.weight"].T + params[p + "dense.bias"]) + att
    return x


def graph_transformer_grads(x, params, gout, dtype, **kw):
    """(out, {name: grad}) of sum(out * gout) on the CPU in ``dtype``."""
    p = {n: torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for n, a in params.items()}
    out = graph_transformer(torch.tensor(np.asarray(x), dtype=dtype), p, **kw)
    out.backward(torch.tensor(np.asarray(gout), dtype=dtype))
    return out.detach().numpy(), {n: a.grad.numpy() for n, a in p.items()}


def asymmetric_graph(M=101, seed=3):
    """A random directed graph: row 5 empty, row 9 one neighbour, row 17 a hub of 40, the others 1 - 6 out-edges."""
    rng = np.random.default_rng(seed)
    A = sparse.lil_matrix((M, M))
    for i in range(M):
        n = {5: 0, 9: 1, 17: 40}.get(i, int(rng.integers(1, 7)))
        for j in rng.choice(M, size=n, replace=False):
            A[i, int(j)] = 1.0
    return A.tocsr()
