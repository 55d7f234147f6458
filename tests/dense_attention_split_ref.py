"""Emulation of the two bf16 split arithmetics of the dense-attention kernels (helper, not collected by pytest).

It models operand rounding only, which is what separates the split kernels from the fp32 ones: every operand of a matrix product is
split as the kernel splits it -- term after term the round-to-nearest bfloat16 (torch's cast) of the running remainder, the
remainder taken in float32, where it is exact -- and the partial products the kernel issues are summed in float64:

    "bf16x3"   a = hi + lo         hi.hi + hi.lo + lo.hi
    "bf16x6"   a = hi + mid + lo   hh + hm + mh + hl + lh + mm

Softmax, lse, P, dP and dS are float64; P and dS are rounded to float32 before their own split, as the kernel holds them.  The
probabilities enter the second product relative to the row's final maximum (the kernel: the running one).
"""

import numpy as np
import torch

TERMS = {"bf16x3": 2, "bf16x6": 3}


def split(a, terms):
    """float32 array -> list of ``terms`` float64 arrays, each a bfloat16 value: a = sum + what the split drops."""
    r = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32))
    parts = []
    for _ in range(terms):
        t = r.to(torch.bfloat16).to(torch.float32)
        parts.append(t.numpy().astype(np.float64))
        r = r - t
    return parts


def split_matmul(a, b, terms):
    """a @ b over the partial products of the arithmetic (term indices i + j < terms), summed in float64."""
    pa, pb = split(a, terms), split(b, terms)
    return sum(pa[i] @ pb[j] for i in range(terms) for j in range(terms) if i + j < terms)


def attention(q, k, v, num_heads, precision, gout=None):
    """q, k, v (N, M, d) float32 -> (out, lse), and with the upstream gradient ``gout`` -> (out, lse, dq, dk, dv); float64."""
    terms = TERMS[precision]
    q, k, v = (np.asarray(t, dtype=np.float32) for t in (q, k, v))
    N, M, d = q.shape
    D = d // num_heads

    def heads_first(t):
        return t.reshape(N, M, num_heads, D).transpose(0, 2, 1, 3)  # (N, heads, M, D)

    def rows_first(t):
        return t.transpose(0, 2, 1, 3).reshape(N, M, d)

    def t_(a):
        return a.transpose(0, 1, 3, 2)

    q4, k4, v4 = heads_first(q), heads_first(k), heads_first(v)
    scale = 1.0 / np.sqrt(D)
    s = split_matmul(q4, t_(k4), terms) * scale
    mx = s.max(-1, keepdims=True)
    e = np.exp(s - mx)
    den = e.sum(-1, keepdims=True)
    out4 = split_matmul(e.astype(np.float32), v4, terms) / den
    lse4 = mx + np.log(den)  # (N, heads, M, 1)
    out, lse = rows_first(out4), lse4[..., 0].transpose(0, 2, 1)
    if gout is None:
        return out, lse
    g4 = heads_first(np.asarray(gout, dtype=np.float32))
    p = np.exp(s - lse4)
    dp = split_matmul(g4, t_(v4), terms)
    delta = (g4.astype(np.float64) * out4).sum(-1, keepdims=True)
    ds = (p * (dp - delta)).astype(np.float32)
    dq4 = split_matmul(ds, k4, terms) * scale
    dk4 = split_matmul(t_(ds), q4, terms) * scale
    dv4 = split_matmul(t_(p.astype(np.float32)), g4, terms)
    return out, lse, rows_first(dq4), rows_first(dk4), rows_first(dv4)
