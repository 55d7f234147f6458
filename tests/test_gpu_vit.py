"""GPU tests of the dense-attention kernels and of Graph_ViT / Healpy_ViT built on them (``pytest -m gpu``).

Reference: tests/dense_attention_ref.py, the reference's materialised-logits algorithm restated in float64.  Error measure:
helpers.rel_err (max |a - b| / max |b|).  Tolerances: 1e-5 forward (out and lse) and 2e-5 gradients, the project's fp32
tolerances (torch fp32 on the CPU sits at <= 1.2e-6 on these inputs); 1e-4 for the large-logit case (torch fp32 on the CPU:
<= 1.1e-5); the whole layer, whose GEMMs and norms are the library's, ten times the error the same layer shows in torch fp32 on
the CPU, computed in the test.  N = 2 throughout (N = 1 in the memory test).  The kernels' tiles are 64 rows: M = 48 is less than
one, 65 one past one (the 260-pixel cap of nside 8 at p = 1), 192 an exact multiple, 331 several plus a ragged tail.

The kernels have three code paths by depth: float4 fragments for D >= 16, float2 fragments and zero-padded A rows for D = 8,
scalar fragments and a 4-float LDS row for D = 4.  Each is run forward and backward, off the tile grid (65, 331) and, backward, at
M = 2, the smallest map whose dq and dk are not identically zero (with one row the softmax is the constant 1).
"""

import functools

import numpy as np
import pytest
import torch

import deepsphere
import dense_attention_ref as ref
from deepsphere import _native, gnn_transformers
from deepsphere.healpy_layers import Healpy_Transformer, Healpy_ViT, HealpyChebyshev
from helpers import offset_view, padded_view, rel_err

pytestmark = pytest.mark.gpu

N = 2
SHAPES = [(1, 4), (4, 16), (2, 64), (3, 16), (4, 64)]
SIZES = [48, 65, 192, 331]


@functools.lru_cache(maxsize=None)
def inputs(M, d, seed=0, scale=1.0):
    rng = np.random.default_rng(seed)
    q, k, v, g = (rng.standard_normal((N, M, d)).astype(np.float32) for _ in range(4))
    return q * np.float32(scale), k * np.float32(scale), v, g


@functools.lru_cache(maxsize=None)
def forward_reference(M, heads, depth, seed=0, scale=1.0):
    q, k, v, _ = inputs(M, heads * depth, seed, scale)
    return ref.attention_np(q, k, v, heads)


def run_forward(q, k, v, heads):
    out, lse = _native.dense_attention(torch.as_tensor(q).cuda(), torch.as_tensor(k).cuda(), torch.as_tensor(v).cuda(), heads)
    torch.cuda.synchronize()
    return out.cpu().numpy(), lse.cpu().numpy()


@pytest.mark.parametrize("heads,depth", SHAPES)
@pytest.mark.parametrize("M", SIZES)
def test_forward_parity(M, heads, depth):
    q, k, v, _ = inputs(M, heads * depth)
    want, _, want_lse = forward_reference(M, heads, depth)
    out, lse = run_forward(q, k, v, heads)
    e_out, e_lse = rel_err(out, want), rel_err(lse, want_lse)
    print(f"M {M} heads {heads} depth {depth}: out {e_out:.2e} lse {e_lse:.2e}")
    assert e_out <= 1e-5 and e_lse <= 1e-5


@pytest.mark.parametrize("heads,depth", [(1, 8), (2, 32)])
@pytest.mark.parametrize("M", [1, 64])
def test_forward_single_row_exact_tile_and_the_other_depths(M, heads, depth):
    """One row (the softmax of one logit: out = v exactly up to 1 / 1), exactly one tile, and the depths 8 and 32 the main matrix
    does not visit."""
    q, k, v, _ = inputs(M, heads * depth)
    want, _, want_lse = forward_reference(M, heads, depth)
    out, lse = run_forward(q, k, v, heads)
    e_out, e_lse = rel_err(out, want), rel_err(lse, want_lse)
    print(f"M {M} heads {heads} depth {depth}: out {e_out:.2e} lse {e_lse:.2e}")
    assert e_out <= 1e-5 and e_lse <= 1e-5


@pytest.mark.parametrize("heads,depth", [(3, 8), (2, 32)])
@pytest.mark.parametrize("M", [48, 65, 331])
def test_forward_depths_8_and_32_off_the_tile_grid(M, heads, depth):
    """The float2 path (D = 8) and two 16-channel blocks (D = 32) with a ragged tail and more than one key tile."""
    q, k, v, _ = inputs(M, heads * depth)
    want, _, want_lse = forward_reference(M, heads, depth)
    out, lse = run_forward(q, k, v, heads)
    e_out, e_lse = rel_err(out, want), rel_err(lse, want_lse)
    print(f"M {M} heads {heads} depth {depth}: out {e_out:.2e} lse {e_lse:.2e}")
    assert e_out <= 1e-5 and e_lse <= 1e-5


def _backward_twice(q, k, v, g, heads):
    runs = []
    for _ in range(2):
        t = [torch.as_tensor(a).cuda().requires_grad_(True) for a in (q, k, v)]
        out = gnn_transformers.scaled_dot_product_attention(t[0], t[1], t[2], heads)
        out.backward(torch.as_tensor(g).cuda())
        torch.cuda.synchronize()
        runs.append([out.detach()] + [a.grad for a in t])
    return runs


@pytest.mark.parametrize("heads,depth", [(1, 4), (3, 4), (3, 8), (1, 8), (2, 32)])
@pytest.mark.parametrize("M", [2, 65, 331])
def test_backward_parity_and_reproducibility_on_the_narrow_paths(M, heads, depth):
    """The backward of the D = 4 and D = 8 paths (and of D = 32), never compared with anything before: same reference, same
    tolerances and the same bit-for-bit repeat as the test below."""
    q, k, v, g = inputs(M, heads * depth)
    want = ref.attention_grads64(q, k, v, heads, g)
    runs = _backward_twice(q, k, v, g, heads)
    errs = [rel_err(a.cpu().numpy(), b) for a, b in zip(runs[0], want)]
    print(f"M {M} heads {heads} depth {depth}: out {errs[0]:.2e} dq {errs[1]:.2e} dk {errs[2]:.2e} dv {errs[3]:.2e}")
    assert np.abs(want[1]).max() > 0 and np.abs(want[2]).max() > 0
    assert errs[0] <= 1e-5 and max(errs[1:]) <= 2e-5
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)  # no atomics: bit for bit


@pytest.mark.parametrize("heads,depth", [(4, 16), (2, 64)])
@pytest.mark.parametrize("M", [65, 331])
def test_backward_parity_and_reproducibility(M, heads, depth):
    q, k, v, g = inputs(M, heads * depth)
    want = ref.attention_grads64(q, k, v, heads, g)
    runs = []
    for _ in range(2):
        t = [torch.as_tensor(a).cuda().requires_grad_(True) for a in (q, k, v)]
        out = gnn_transformers.scaled_dot_product_attention(t[0], t[1], t[2], heads)
        out.backward(torch.as_tensor(g).cuda())
        torch.cuda.synchronize()
        runs.append([out.detach()] + [a.grad for a in t])
    errs = [rel_err(a.cpu().numpy(), b) for a, b in zip(runs[0], want)]
    print(f"M {M} heads {heads} depth {depth}: out {errs[0]:.2e} dq {errs[1]:.2e} dk {errs[2]:.2e} dv {errs[3]:.2e}")
    assert errs[0] <= 1e-5 and max(errs[1:]) <= 2e-5
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)  # no atomics: bit for bit


def test_strided_views_are_bitwise_the_contiguous_result():
    M, heads, depth = 65, 4, 16
    d = heads * depth
    buf = torch.as_tensor(np.random.default_rng(1).standard_normal((N, M, 3 * d)).astype(np.float32)).cuda()
    q, k, v = buf[..., :d], buf[..., d:2 * d], buf[..., 2 * d:]
    assert _native.rows_layout(k) == 3 * d and not k.is_contiguous()
    o_view, l_view = _native.dense_attention(q, k, v, heads)
    o_copy, l_copy = _native.dense_attention(q.contiguous(), k.contiguous(), v.contiguous(), heads)
    assert torch.equal(o_view, o_copy) and torch.equal(l_view, l_copy)
    # and through the packed differentiable op: one gradient tensor, equal to the three gradients of the copies side by side
    g = torch.as_tensor(inputs(M, d)[3]).cuda()
    leaf = buf.clone().requires_grad_(True)
    out_p = gnn_transformers._DenseAttentionPacked.apply(leaf, heads)
    out_p.backward(g)
    t = [a.clone().contiguous().requires_grad_(True) for a in (q, k, v)]
    out_c = gnn_transformers.scaled_dot_product_attention(t[0], t[1], t[2], heads)
    out_c.backward(g)
    assert torch.equal(out_p, out_c) and torch.equal(out_p, o_view)
    assert tuple(leaf.grad.shape) == (N, M, 3 * d) and torch.equal(leaf.grad, torch.cat([a.grad for a in t], dim=2))
    # views into the unpacked op give the same gradients too
    leaf2 = buf.clone().requires_grad_(True)
    gnn_transformers.scaled_dot_product_attention(leaf2[..., :d], leaf2[..., d:2 * d], leaf2[..., 2 * d:], heads).backward(g)
    assert torch.equal(leaf2.grad, leaf.grad)


@pytest.mark.parametrize("heads,depth", [(3, 8), (1, 4)])
def test_packed_op_on_the_narrow_paths_is_bitwise_the_contiguous_result(heads, depth):
    """``_DenseAttentionPacked`` on a (N, M, 3 d) buffer: the D = 8 path reads float2 and the D = 4 path scalars through the
    strided views; one gradient tensor, equal bit for bit to the three gradients of the contiguous copies side by side."""
    M, d = 65, heads * depth
    buf = torch.as_tensor(np.random.default_rng(1).standard_normal((N, M, 3 * d)).astype(np.float32)).cuda()
    q, k, v = buf[..., :d], buf[..., d:2 * d], buf[..., 2 * d:]
    assert _native.rows_layout(k) == 3 * d and not k.is_contiguous() and all(a.data_ptr() % 16 == 0 for a in (q, k, v))
    o_view, l_view = _native.dense_attention(q, k, v, heads)
    o_copy, l_copy = _native.dense_attention(q.contiguous(), k.contiguous(), v.contiguous(), heads)
    assert torch.equal(o_view, o_copy) and torch.equal(l_view, l_copy)
    g = torch.as_tensor(inputs(M, d)[3]).cuda()
    leaf = buf.clone().requires_grad_(True)
    out_p = gnn_transformers._DenseAttentionPacked.apply(leaf, heads)
    out_p.backward(g)
    t = [a.clone().contiguous().requires_grad_(True) for a in (q, k, v)]
    out_c = gnn_transformers.scaled_dot_product_attention(t[0], t[1], t[2], heads)
    out_c.backward(g)
    assert torch.equal(out_p, out_c) and torch.equal(out_p, o_view)
    assert tuple(leaf.grad.shape) == (N, M, 3 * d) and torch.equal(leaf.grad, torch.cat([a.grad for a in t], dim=2))
    # and the packed result is the right one, not merely the same one
    want = ref.attention_grads64(*(a.cpu().numpy() for a in (q, k, v)), heads, g.cpu().numpy())
    errs = [rel_err(out_p.detach().cpu().numpy(), want[0])] + [rel_err(leaf.grad[..., i * d:(i + 1) * d].cpu().numpy(), want[1 + i])
                                                               for i in range(3)]
    print(f"packed heads {heads} depth {depth}: out {errs[0]:.2e} dq {errs[1]:.2e} dk {errs[2]:.2e} dv {errs[3]:.2e}")
    assert errs[0] <= 1e-5 and max(errs[1:]) <= 2e-5


def test_misaligned_views_are_refused_before_any_launch():
    """As test_gpu_attention's: a storage offset of one float and a row stride that is no multiple of four floats are refused by
    the C ABI, forward and backward, before anything is launched.  ``_native.dense_attention`` raises the C ABI's error; the
    differentiable op copies a badly strided view (and then gives the contiguous call's bits) and raises on an offset view,
    which is contiguous already, so that a copy changes nothing."""
    M, heads, depth = 65, 2, 8
    d = heads * depth
    q, k, v, g = (torch.as_tensor(a).cuda() for a in inputs(M, d))
    out, lse = _native.dense_attention(q, k, v, heads)
    off = [offset_view(a, 1) for a in (q, k, v)]
    pad = [padded_view(a, 2) for a in (q, k, v)]
    assert _native.rows_layout(pad[0]) == d + 2 and (d + 2) % 4 != 0
    with pytest.raises(ValueError, match="must be 16-byte aligned"):
        _native.dense_attention(off[0], off[1], off[2], heads)
    with pytest.raises(ValueError, match="row stride 18 must be a multiple of 4 floats"):
        _native.dense_attention(pad[0], pad[1], pad[2], heads)
    with pytest.raises(ValueError, match="must be 16-byte aligned"):
        _native.dense_attention_backward(off[0], off[1], off[2], out, lse, g, heads)
    with pytest.raises(ValueError, match="row stride 18 must be a multiple of 4 floats"):
        _native.dense_attention_backward(pad[0], pad[1], pad[2], out, lse, g, heads)

    L, p, stream = _native.lib(), _native._ptr, _native._stream_ptr(q.device)
    o_fill, l_fill = torch.full_like(out, 7.0), torch.full_like(lse, 7.0)
    grads = [torch.full_like(out, 7.0) for _ in range(3)]
    delta = torch.full_like(lse, 7.0)
    for views, ld, text in ((off, d, "16-byte aligned"), (pad, d + 2, "multiple of 4 floats")):
        rc = L.dsph_dense_attention_forward(p(views[0]), p(views[1]), p(views[2]), ld, p(o_fill), p(l_fill), N, M, heads, depth, 0, stream)
        assert rc == -1 and text in _native.last_error()
        rc = L.dsph_dense_attention_backward(p(views[0]), p(views[1]), p(views[2]), ld, p(out), p(lse), p(g), p(delta), p(grads[0]),
                                             p(grads[1]), p(grads[2]), d, N, M, heads, depth, 0, stream)
        assert rc == -1 and text in _native.last_error()
    goff = [offset_view(a, 1) for a in grads]
    rc = L.dsph_dense_attention_backward(p(q), p(k), p(v), d, p(out), p(lse), p(g), p(delta), p(goff[0]), p(goff[1]), p(goff[2]), d, N, M,
                                         heads, depth, 0, stream)
    assert rc == -1 and "16-byte aligned" in _native.last_error()
    torch.cuda.synchronize()
    for t in [o_fill, l_fill, delta] + grads + goff:
        assert bool((t == 7.0).all())  # nothing ran

    with pytest.raises(ValueError, match="must be 16-byte aligned"):
        gnn_transformers.scaled_dot_product_attention(off[0], off[1], off[2], heads)
    results = []
    for src in ((q, k, v), pad):
        t = [a.detach().requires_grad_(True) for a in src]
        o = gnn_transformers.scaled_dot_product_attention(t[0], t[1], t[2], heads)
        o.backward(g)
        results.append([o.detach()] + [a.grad for a in t])
    assert torch.equal(results[0][0], out)
    for a, b in zip(results[0], results[1]):
        assert torch.equal(a, b)  # the copies: bit for bit the contiguous call


def test_large_logits_do_not_overflow():
    M, heads, depth = 192, 2, 16
    q, k, v, _ = inputs(M, heads * depth, seed=7, scale=6.0)
    want, s, want_lse = forward_reference(M, heads, depth, seed=7, scale=6.0)
    assert s.max() > 100 and np.isfinite(want).all()  # exp of the raw logit overflows in fp32 (above 88), not in float64
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(s.astype(np.float32))).any()
    out, lse = run_forward(q, k, v, heads)
    err, err_lse = rel_err(out, want), rel_err(lse, want_lse)
    print(f"logits in [{s.min():.0f}, {s.max():.0f}]: out {err:.2e} lse {err_lse:.2e}")
    assert np.isfinite(out).all() and np.isfinite(lse).all() and err <= 1e-4


def test_nothing_of_size_m_squared_is_allocated():
    """12,288 tokens (nside 128 at p = 1): forward + backward hold about ten tensors the size of q; one head's logits of one map
    would be 400 times q."""
    M, heads, depth = 12288, 2, 16
    d = heads * depth
    gen = torch.Generator(device="cuda").manual_seed(3)
    t = [torch.randn((1, M, d), generator=gen, device="cuda").requires_grad_(True) for _ in range(3)]
    g = torch.randn((1, M, d), generator=gen, device="cuda")
    q_bytes = M * d * 4
    assert M * M * 4 == 384 * q_bytes
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = gnn_transformers.scaled_dot_product_attention(t[0], t[1], t[2], heads)
    out.backward(g)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f"M {M}: peak grew by {grown / q_bytes:.1f} x the bytes of q")
    assert grown < 16 * q_bytes
    assert all(a.grad is not None and torch.isfinite(a.grad).all() for a in t) and torch.isfinite(out).all()


def test_bad_shapes_raise():
    M = 48
    t = torch.zeros((N, M, 24), device="cuda")
    with pytest.raises(ValueError, match="4, 8, 16, 32, 64"):
        _native.dense_attention(t, t, t, 2)  # depth 12
    t = torch.zeros((N, M, 320), device="cuda")
    with pytest.raises(ValueError, match="256"):
        _native.dense_attention(t, t, t, 5)
    t = torch.zeros((N, M, 16), device="cuda")
    with pytest.raises(ValueError, match="one shape"):
        _native.dense_attention(t, torch.zeros((N, M + 1, 16), device="cuda"), t, 1)
    with pytest.raises(ValueError, match="HIP tensors"):
        _native.dense_attention(t.cpu(), t.cpu(), t.cpu(), 1)
    with pytest.raises(ValueError, match="no CPU path"):
        gnn_transformers.scaled_dot_product_attention(t.cpu(), t.cpu(), t.cpu(), 1)
    out, lse = _native.dense_attention(t, t, t, 1)
    with pytest.raises(ValueError, match="4, 8, 16, 32, 64"):
        bad = torch.zeros((N, M, 24), device="cuda")
        _native.dense_attention_backward(bad, bad, bad, bad, torch.zeros((N, M, 2), device="cuda"), bad, 2)
    with pytest.raises(ValueError, match="forward's shapes"):
        _native.dense_attention_backward(t, t, t, out, lse[:, :-1], out, 1)


def _randomise(layer, seed):
    """Every parameter away from its special initial value (zero biases, unit gains), seeded (as test_gpu_attention._randomise)."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in layer.named_parameters():
            r = torch.randn(p.shape, generator=gen)
            if name.endswith("bias") or "pos_embedding" in name:
                p.copy_((0.3 * r).to(p.device))
            elif "layer_norm" in name:
                p.copy_((1.0 + 0.2 * r).to(p.device))
            else:
                p.copy_((r / np.sqrt(p.shape[1])).to(p.device))


@pytest.mark.parametrize("layer_norm,positional_encoding", [(True, True), (False, True), (True, False)])
def test_graph_vit_end_to_end(layer_norm, positional_encoding):
    M, p, Fin, key_dim, heads, n_layers = 192, 1, 5, 8, 2, 2
    layer = gnn_transformers.Graph_ViT(p, key_dim, heads, positional_encoding=positional_encoding, n_layers=n_layers,
                                       layer_norm=layer_norm)
    rng = np.random.default_rng(11)
    x = rng.standard_normal((N, M, Fin)).astype(np.float32)
    g = rng.standard_normal((N, M // 4, key_dim * heads)).astype(np.float32)
    xg = torch.as_tensor(x).cuda()
    with torch.no_grad():
        layer(xg)  # builds the lazily created parameters
    _randomise(layer, 5)
    names = [n for n, _ in layer.named_parameters()]
    assert "embed.weight" in names and "embed.bias" in names and ("pos_encoder.pos_embedding" in names) == positional_encoding
    assert ("mha_layers.1.layer_norm2.weight" in names) == layer_norm and "mha_layers.1.wqkv.weight" in names
    assert tuple(layer.embed.weight.shape) == (key_dim * heads, Fin, 4)
    if positional_encoding:
        assert tuple(layer.pos_encoder.pos_embedding.shape) == (1, M // 4, key_dim * heads)
    out = layer(xg)
    assert tuple(out.shape) == (N, M // 4, key_dim * heads)
    out.backward(torch.as_tensor(g).cuda())
    torch.cuda.synchronize()
    params = {n: q.detach().cpu().numpy() for n, q in layer.named_parameters()}
    kw = dict(p=p, num_heads=heads, n_layers=n_layers, positional_encoding=positional_encoding, layer_norm=layer_norm)
    out64, g64 = ref.graph_vit_grads(x, params, g, torch.float64, **kw)
    out32, g32 = ref.graph_vit_grads(x, params, g, torch.float32, **kw)
    got = {n: q.grad.cpu().numpy() for n, q in layer.named_parameters()}
    e_cpu, e_gpu = rel_err(out32, out64), rel_err(out.detach().cpu().numpy(), out64)
    print(f"norm {layer_norm} pos {positional_encoding}: output cpu-fp32 {e_cpu:.2e} gpu {e_gpu:.2e}")
    failed = [] if e_gpu <= 10 * e_cpu else [("output", e_gpu, e_cpu)]
    for n in names:
        e_cpu, e_gpu = rel_err(g32[n], g64[n]), rel_err(got[n], g64[n])
        print(f"  d {n}: cpu-fp32 {e_cpu:.2e} gpu {e_gpu:.2e}")
        if not e_gpu <= 10 * e_cpu:
            failed.append((n, e_gpu, e_cpu))
    assert not failed, f"more than ten times the CPU fp32 error: {failed}"


def test_healpy_gcnn_composition():
    model = deepsphere.HealpyGCNN(8, np.arange(768), [HealpyChebyshev(K=3, Fout=8), Healpy_ViT(1, 8, 2), Healpy_Transformer(8, 2)])
    x = torch.as_tensor(np.random.default_rng(2).standard_normal((N, 768, 3)).astype(np.float32)).cuda()
    with torch.no_grad():
        y = model(x)
        z = x
        for layer in model:
            z = layer(z)
    assert tuple(y.shape) == (N, 192, 16) and torch.isfinite(y).all()
    assert isinstance(model[1], gnn_transformers.Graph_ViT) and isinstance(model[2], gnn_transformers.Graph_Transformer)
    assert model[2].nbr.shape[0] == 192  # the transformer after the ViT works on the graph of the reduced map
    assert torch.equal(y, z)
    # and it trains: gradients reach the ViT's embedding through the transformer behind it
    model(x, training=True).square().sum().backward()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in model[1].parameters())
    assert float(model[1].embed.weight.grad.abs().max()) > 0
