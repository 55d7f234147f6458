"""GPU tests of the dense attention's bf16 split arithmetics, ``precision="bf16x6" | "bf16x3"`` (``pytest -m gpu``).

Reference: tests/dense_attention_ref.py in float64.  Error measure: helpers.rel_err.  N = 2 (N = 1 in the memory test).

Tolerances.  T_fp32 = 1e-5 (out, lse), 2e-5 (dq, dk, dv), 1e-4 (out at large logits): those of tests/test_gpu_vit.py.
  "bf16x6" is held to T_fp32 as it stands: the six-term split is fp32-equivalent (its emulation sits two orders below).
  "bf16x3" is held to T_fp32 + 3 E_emul, E_emul being the error of the numpy emulation of the arithmetic
  (tests/dense_attention_split_ref.py: operand rounding only, products in float64) on the same inputs against the same
  reference, computed here on the CPU.  T_fp32 covers what the emulation leaves out (fp32 accumulation order, exp); the factor 3
  covers a different realisation of the same rounding (the kernel splits p relative to the running maximum, the emulation
  relative to the final one).  A mis-built emulation must not loosen the bound: E_emul above 1e-4 at unit scale, or above 1e-3
  at large logits, on any quantity fails the test.

Shapes, the smallest that reach each path: (heads, depth) = (2, 32), (1, 64), (4, 64) -- both depths, one and two K = 32 steps of
the first product, the 256-channel limit; M = 2 (the smallest map with non-zero dq / dk), 64 (one exact tile of 64 rows, two of
the 32-row tiles the depth-64 backward streams), 65 (one row past), 331 (several tiles and a ragged tail), forward also M = 1.
"""

import functools

import numpy as np
import pytest
import torch

import deepsphere
import dense_attention_ref as ref
import dense_attention_split_ref as split_ref
from deepsphere import _native, gnn_transformers
from deepsphere.healpy_layers import Healpy_ViT
from helpers import rel_err

pytestmark = pytest.mark.gpu

N = 2
SHAPES = [(2, 32), (1, 64), (4, 64)]
PRECISIONS = ["bf16x6", "bf16x3"]
CODES = {"fp32": _native.PREC_FP32, "bf16x6": _native.PREC_BF16X6, "bf16x3": _native.PREC_BF16X3}
T_OUT, T_GRAD, T_LARGE = 1e-5, 2e-5, 1e-4
EMUL_CAP, EMUL_CAP_LARGE = 1e-4, 1e-3


@functools.lru_cache(maxsize=None)
def inputs(M, d, seed=0, scale=1.0):
    rng = np.random.default_rng(seed)
    q, k, v, g = (rng.standard_normal((N, M, d)).astype(np.float32) for _ in range(4))
    return q * np.float32(scale), k * np.float32(scale), v, g


@functools.lru_cache(maxsize=None)
def forward_reference(M, heads, depth, seed=0, scale=1.0):
    q, k, v, _ = inputs(M, heads * depth, seed, scale)
    return ref.attention_np(q, k, v, heads)  # out, logits, lse


@functools.lru_cache(maxsize=None)
def backward_reference(M, heads, depth):
    q, k, v, g = inputs(M, heads * depth)
    return ref.attention_grads64(q, k, v, heads, g)  # out, dq, dk, dv


@functools.lru_cache(maxsize=None)
def emulation_errors(M, heads, depth, precision, backward, seed=0, scale=1.0):
    """E_emul per quantity: (out, lse) or, with ``backward``, (out, dq, dk, dv); 0 for "bf16x6", whose bound takes no allowance."""
    if precision == "bf16x6":
        return (0.0,) * (4 if backward else 2)
    q, k, v, g = inputs(M, heads * depth, seed, scale)
    cap = EMUL_CAP if scale == 1.0 else EMUL_CAP_LARGE
    if backward:
        emul = split_ref.attention(q, k, v, heads, precision, g)
        errs = tuple(rel_err(emul[i], w) for i, w in zip((0, 2, 3, 4), backward_reference(M, heads, depth)))
    else:
        want, _, want_lse = forward_reference(M, heads, depth, seed, scale)
        out, lse = split_ref.attention(q, k, v, heads, precision)
        errs = (rel_err(out, want), rel_err(lse, want_lse))
    print(f"emulation {precision} M {M} heads {heads} depth {depth}: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= cap, f"the emulation itself is off by {errs}: it would loosen the bound"
    return errs


def run_forward(q, k, v, heads, precision):
    out, lse = _native.dense_attention(torch.as_tensor(q).cuda(), torch.as_tensor(k).cuda(), torch.as_tensor(v).cuda(), heads,
                                       precision=CODES[precision])
    torch.cuda.synchronize()
    return out.cpu().numpy(), lse.cpu().numpy()


def run_backward(q, k, v, g, heads, precision):
    t = [torch.as_tensor(a).cuda().requires_grad_(True) for a in (q, k, v)]
    out = gnn_transformers.scaled_dot_product_attention(t[0], t[1], t[2], heads, precision=precision)
    out.backward(torch.as_tensor(g).cuda())
    torch.cuda.synchronize()
    return [out.detach()] + [a.grad for a in t]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("heads,depth", SHAPES)
@pytest.mark.parametrize("M", [1, 2, 64, 65, 331])
def test_forward_parity(M, heads, depth, precision):
    q, k, v, _ = inputs(M, heads * depth)
    want, _, want_lse = forward_reference(M, heads, depth)
    e_emul = emulation_errors(M, heads, depth, precision, False)
    out, lse = run_forward(q, k, v, heads, precision)
    e_out, e_lse = rel_err(out, want), rel_err(lse, want_lse)
    print(f"{precision} M {M} heads {heads} depth {depth}: out {e_out:.2e} lse {e_lse:.2e}")
    assert e_out <= T_OUT + 3 * e_emul[0] and e_lse <= T_OUT + 3 * e_emul[1]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("heads,depth", SHAPES)
@pytest.mark.parametrize("M", [2, 64, 65, 331])
def test_backward_parity_and_reproducibility(M, heads, depth, precision):
    q, k, v, g = inputs(M, heads * depth)
    want = backward_reference(M, heads, depth)
    e_emul = emulation_errors(M, heads, depth, precision, True)
    runs = [run_backward(q, k, v, g, heads, precision) for _ in range(2)]
    errs = [rel_err(a.cpu().numpy(), b) for a, b in zip(runs[0], want)]
    print(f"{precision} M {M} heads {heads} depth {depth}: out {errs[0]:.2e} dq {errs[1]:.2e} dk {errs[2]:.2e} dv {errs[3]:.2e}")
    assert np.abs(want[1]).max() > 0 and np.abs(want[2]).max() > 0
    assert errs[0] <= T_OUT + 3 * e_emul[0]
    for e, em in zip(errs[1:], e_emul[1:]):
        assert e <= T_GRAD + 3 * em
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)  # no atomics: bit for bit


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("heads,depth", [(2, 32), (1, 64)])
def test_packed_op_is_bitwise_the_contiguous_result(heads, depth, precision):
    """``_DenseAttentionPacked`` on an (N, 65, 3 d) buffer: three strided views read in place, one gradient tensor, bit for bit the
    op on contiguous copies and its three gradients side by side."""
    M, d, code = 65, heads * depth, CODES[precision]
    buf = torch.as_tensor(np.random.default_rng(1).standard_normal((N, M, 3 * d)).astype(np.float32)).cuda()
    q, k, v = buf[..., :d], buf[..., d:2 * d], buf[..., 2 * d:]
    assert _native.rows_layout(k) == 3 * d and not k.is_contiguous()
    o_view, l_view = _native.dense_attention(q, k, v, heads, precision=code)
    o_copy, l_copy = _native.dense_attention(q.contiguous(), k.contiguous(), v.contiguous(), heads, precision=code)
    assert torch.equal(o_view, o_copy) and torch.equal(l_view, l_copy)
    g = torch.as_tensor(inputs(M, d)[3]).cuda()
    leaf = buf.clone().requires_grad_(True)
    out_p = gnn_transformers._DenseAttentionPacked.apply(leaf, heads, code)
    out_p.backward(g)
    t = [a.clone().contiguous().requires_grad_(True) for a in (q, k, v)]
    out_c = gnn_transformers.scaled_dot_product_attention(t[0], t[1], t[2], heads, precision=precision)
    out_c.backward(g)
    assert torch.equal(out_p, out_c) and torch.equal(out_p, o_view)
    assert tuple(leaf.grad.shape) == (N, M, 3 * d) and torch.equal(leaf.grad, torch.cat([a.grad for a in t], dim=2))
    # and it is the arithmetic asked for, not the fp32 one: the packed fp32 result differs
    out_f = gnn_transformers._DenseAttentionPacked.apply(buf.clone(), heads)
    assert not torch.equal(out_f, out_p)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_large_logits_do_not_overflow(precision):
    M, heads, depth = 192, 2, 32
    q, k, v, _ = inputs(M, heads * depth, seed=7, scale=6.0)
    want, s, want_lse = forward_reference(M, heads, depth, seed=7, scale=6.0)
    assert s.max() > 100 and np.isfinite(want).all()  # exp of the raw logit overflows in fp32 (above 88), not in float64
    e_emul = emulation_errors(M, heads, depth, precision, False, seed=7, scale=6.0)
    out, lse = run_forward(q, k, v, heads, precision)
    err, err_lse = rel_err(out, want), rel_err(lse, want_lse)
    print(f"{precision} logits in [{s.min():.0f}, {s.max():.0f}]: out {err:.2e} lse {err_lse:.2e}")
    assert np.isfinite(out).all() and np.isfinite(lse).all()
    assert err <= T_LARGE + 3 * e_emul[0] and err_lse <= T_OUT + 3 * e_emul[1]


def test_fp32_through_the_new_entry_points_is_the_old_kernels_and_a_split_is_not():
    M, heads, depth = 331, 2, 32
    d = heads * depth
    q, k, v, g = (torch.as_tensor(a).cuda() for a in inputs(M, d))
    L, p, stream = _native.lib(), _native._ptr, _native._stream_ptr(q.device)
    out_old, lse_old = torch.empty_like(q), torch.empty((N, M, heads), device="cuda")
    rc = L.dsph_dense_attention_forward(p(q), p(k), p(v), d, p(out_old), p(lse_old), N, M, heads, depth, 0, stream)
    assert rc == 0
    grads_old, delta = [torch.empty_like(q) for _ in range(3)], torch.empty_like(lse_old)
    rc = L.dsph_dense_attention_backward(p(q), p(k), p(v), d, p(out_old), p(lse_old), p(g), p(delta), p(grads_old[0]), p(grads_old[1]),
                                         p(grads_old[2]), d, N, M, heads, depth, 0, stream)
    assert rc == 0
    out_new, lse_new = _native.dense_attention(q, k, v, heads, precision=_native.PREC_FP32)
    grads_new = _native.dense_attention_backward(q, k, v, out_new, lse_new, g, heads, precision=_native.PREC_FP32)
    torch.cuda.synchronize()
    assert torch.equal(out_new, out_old) and torch.equal(lse_new, lse_old)
    for a, b in zip(grads_new, grads_old):
        assert torch.equal(a, b)
    for precision in PRECISIONS:  # (the fp32 kernel must not answer under another name)
        out_s, lse_s = _native.dense_attention(q, k, v, heads, precision=CODES[precision])
        grads_s = _native.dense_attention_backward(q, k, v, out_s, lse_s, g, heads, precision=CODES[precision])
        torch.cuda.synchronize()
        assert not torch.equal(out_s, out_old)
        assert not any(torch.equal(a, b) for a, b in zip(grads_s, grads_old))
    out_3, _ = _native.dense_attention(q, k, v, heads, precision=_native.PREC_BF16X3)
    out_6, _ = _native.dense_attention(q, k, v, heads, precision=_native.PREC_BF16X6)
    assert not torch.equal(out_3, out_6)


def test_split_at_other_depths_is_refused_before_any_launch():
    M, heads, depth = 48, 2, 16
    d = heads * depth
    q, k, v, g = (torch.as_tensor(a).cuda() for a in inputs(M, d))
    out, lse = _native.dense_attention(q, k, v, heads)
    for code in (_native.PREC_BF16X6, _native.PREC_BF16X3):
        with pytest.raises(RuntimeError, match="32, 64"):
            _native.dense_attention(q, k, v, heads, precision=code)
        with pytest.raises(RuntimeError, match="32, 64"):
            _native.dense_attention_backward(q, k, v, out, lse, g, heads, precision=code)
    with pytest.raises(ValueError, match="'fp32', 'bf16x6', 'bf16x3'"):
        gnn_transformers.scaled_dot_product_attention(q, k, v, heads, precision="bf16")
    with pytest.raises(ValueError, match="precision"):
        _native.dense_attention(q, k, v, heads, precision=99)
    L, p, stream = _native.lib(), _native._ptr, _native._stream_ptr(q.device)
    o_fill, l_fill, delta = torch.full_like(out, 7.0), torch.full_like(lse, 7.0), torch.full_like(lse, 7.0)
    grads = [torch.full_like(out, 7.0) for _ in range(3)]
    for code, want_rc in ((_native.PREC_BF16X6, -3), (_native.PREC_BF16X3, -3), (99, -1)):
        rc = L.dsph_dense_attention_forward_prec(p(q), p(k), p(v), d, p(o_fill), p(l_fill), N, M, heads, depth, code, 0, stream)
        assert rc == want_rc
        rc = L.dsph_dense_attention_backward_prec(p(q), p(k), p(v), d, p(out), p(lse), p(g), p(delta), p(grads[0]), p(grads[1]),
                                                  p(grads[2]), d, N, M, heads, depth, code, 0, stream)
        assert rc == want_rc
    torch.cuda.synchronize()
    for t in [o_fill, l_fill, delta] + grads:
        assert bool((t == 7.0).all())  # nothing ran


def _randomise(layer, seed):
    """Every parameter away from its special initial value (zero biases, unit gains), seeded."""
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


def test_graph_vit_on_the_six_term_split_matches_its_fp32_twin():
    """Graph_ViT(precision="bf16x6") against a precision="fp32" twin with the same parameters: outputs and input gradients agree
    to ten times the error the fp32 twin shows against the same layer in torch float64 on the CPU."""
    M, p, Fin, key_dim, heads, n_layers = 192, 1, 3, 32, 2, 2
    layer = gnn_transformers.Graph_ViT(p, key_dim, heads, n_layers=n_layers, precision="bf16x6")
    twin = gnn_transformers.Graph_ViT(p, key_dim, heads, n_layers=n_layers, precision="fp32")
    assert [m.precision for m in layer.mha_layers] == ["bf16x6"] * 2 and [m.precision for m in twin.mha_layers] == ["fp32"] * 2
    rng = np.random.default_rng(11)
    x = rng.standard_normal((N, M, Fin)).astype(np.float32)
    g = rng.standard_normal((N, M // 4, key_dim * heads)).astype(np.float32)
    with torch.no_grad():
        layer(torch.as_tensor(x).cuda())  # builds the lazily created parameters
        twin(torch.as_tensor(x).cuda())
    _randomise(layer, 5)
    twin.load_state_dict(layer.state_dict())
    results = []
    for m in (layer, twin):
        xg = torch.as_tensor(x).cuda().requires_grad_(True)
        out = m(xg)
        out.backward(torch.as_tensor(g).cuda())
        torch.cuda.synchronize()
        results.append((out.detach().cpu().numpy(), xg.grad.cpu().numpy()))
    params = {n: torch.tensor(q.detach().cpu().numpy(), dtype=torch.float64) for n, q in layer.named_parameters()}
    x64 = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    out64 = ref.graph_vit(x64, params, p=p, num_heads=heads, n_layers=n_layers)
    out64.backward(torch.tensor(g, dtype=torch.float64))
    out64, dx64 = out64.detach().numpy(), x64.grad.numpy()
    (out_s, dx_s), (out_f, dx_f) = results
    for name, got, twin_got, want in (("output", out_s, out_f, out64), ("dx", dx_s, dx_f, dx64)):
        e_twin, e_split, e_between = rel_err(twin_got, want), rel_err(got, want), rel_err(got, twin_got)
        print(f"{name}: fp32 twin vs float64 {e_twin:.2e}, bf16x6 vs float64 {e_split:.2e}, bf16x6 vs twin {e_between:.2e}")
        assert e_between <= 10 * e_twin
    assert not np.array_equal(out_s, out_f)  # the twin ran another kernel


def test_healpy_gcnn_with_a_three_term_vit():
    model = deepsphere.HealpyGCNN(8, np.arange(768), [Healpy_ViT(1, 32, 2, precision="bf16x3")])
    x = torch.as_tensor(np.random.default_rng(2).standard_normal((N, 768, 3)).astype(np.float32)).cuda()
    with torch.no_grad():
        y = model(x)
    assert tuple(y.shape) == (N, 192, 64) and torch.isfinite(y).all()
    assert model[0].mha_layers[0].precision == "bf16x3"


def test_nothing_of_size_m_squared_is_allocated():
    """12,288 tokens: forward + backward on the six-term split hold about ten tensors the size of q, the bound of the fp32 test."""
    M, heads, depth = 12288, 2, 32
    d = heads * depth
    gen = torch.Generator(device="cuda").manual_seed(3)
    t = [torch.randn((1, M, d), generator=gen, device="cuda").requires_grad_(True) for _ in range(3)]
    g = torch.randn((1, M, d), generator=gen, device="cuda")
    q_bytes = M * d * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = gnn_transformers.scaled_dot_product_attention(t[0], t[1], t[2], heads, precision="bf16x6")
    out.backward(g)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print(f"M {M}: peak grew by {grown / q_bytes:.1f} x the bytes of q")
    assert grown < 16 * q_bytes
    assert all(a.grad is not None and torch.isfinite(a.grad).all() for a in t) and torch.isfinite(out).all()
