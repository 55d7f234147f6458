"""GPU tests of the layer-norm kernels (``dsph_ln_forward`` / ``dsph_ln_backward``, csrc/layer_norm.hip) and of the layers on
them (``pytest -m gpu``).

Yardstick: tests/layernorm_ref.py (float64 numpy; held to torch's float64 autograd at 1e-12 by tests/test_layernorm_host.py).
Error measure: ``helpers.rel_err`` (max-norm over max-norm).  Bounds, the sibling kernels' (tests/test_gpu_batchnorm.py): z 1e-5; da,
dgamma, dbeta 2e-5; the sum output is ``torch.equal`` to torch's fp32 x + res (one fp32 add).  Where the reference is identically
zero (dgamma at d = 1: x^ = 0) the absolute error is held to 2e-5 max|dbeta|.

Data (``layernorm_ref.make_data``): seeded rows of N(0, 1) shifted by 0, +10 and -3 in turn, row 4 constant, gamma = 1 + 0.2 N,
beta = 0.3 N.  Every figure is printed before it is asserted.
"""

import functools

import numpy as np
import pytest
import torch
from scipy import sparse

import attention_ref
import dense_attention_ref
import layernorm_ref as ref
from deepsphere import _native, gnn_transformers, healpix
from deepsphere.gnn_layers import GCNN_ResidualLayer, _LayerNormFunction
from helpers import offset_view, rel_err
from oracle import cheb_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-5
TOL_GRAD = 2e-5
EPS = 1e-3

# (rows, d, floats off 16-byte alignment): the smallest shapes at which each path of the kernels can go wrong
SHAPES = [
    (3, 1, 0),       # variance 0 in every row
    (7, 2, 0),       # x^ = +-(1 - e): da is a cancellation
    (130, 5, 0),     # scalar lanes, 8 lanes per row of which 3 idle, a ragged last wave
    (257, 8, 0),     # 2 lanes per row, row tail
    (1000, 16, 0),   # 4 lanes per row
    (4099, 64, 0),   # 16 lanes per row, several workgroups, row tail
    (300, 256, 0),   # one row per wave
    (33, 260, 0),    # 65 vectors on 64 lanes: two per lane, the second almost empty
    (9, 1024, 0),    # four vectors per lane, the widest row
    (515, 100, 1),   # d % 4 == 0 through maps 4 bytes off alignment: the scalar path, two scalars per lane
]
IDS = [f"{r}x{d}" + ("+4B" if o else "") for r, d, o in SHAPES]


def dev(a, offset=0):
    if offset:
        return offset_view(a, offset)
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda()


@functools.lru_cache(maxsize=None)
def data(rows, d):
    """x, res, dz, dsum, gamma, beta (float32 numpy); shared, never written."""
    return ref.make_data(rows, d)


@functools.lru_cache(maxsize=None)
def yardstick(rows, d, with_res, affine):
    x, res, dz, dsum, gamma, beta = data(rows, d)
    g, b = (gamma, beta) if affine else (None, None)
    z, a = ref.ln_forward(x, EPS, g, b, res if with_res else None)
    a32 = (x + res) if with_res else x  # what the backward is handed: the fp32 sum
    da, dgamma, dbeta = ref.ln_backward(a32, dz, EPS, g, dsum if with_res else None)
    assert np.isfinite(z).all() and np.isfinite(da).all()
    return z, a32, da, dgamma, dbeta


def grad_errs(d, da, dgamma, dbeta, want):
    _, _, da_ref, dg_ref, db_ref = want
    errs = {"da": rel_err(da.cpu().numpy(), da_ref)}
    if dbeta is not None:
        errs["dbeta"] = rel_err(dbeta.cpu().numpy(), db_ref)
    if dgamma is not None:
        if d == 1:  # the reference is identically zero
            errs["dgamma(abs)"] = float(np.abs(dgamma.cpu().numpy().astype(np.float64) - dg_ref).max() / np.abs(db_ref).max())
        else:
            errs["dgamma"] = rel_err(dgamma.cpu().numpy(), dg_ref)
    return errs


@pytest.mark.parametrize("affine", [True, False], ids=["gamma+beta", "plain"])
@pytest.mark.parametrize("with_res", [True, False], ids=["res", "no-res"])
@pytest.mark.parametrize("rows,d,offset", SHAPES, ids=IDS)
def test_kernels_against_the_float64_yardstick(rows, d, offset, with_res, affine):
    """Measured on an MI355X, largest over all cases: z 6.4e-7 (at (130, 5) with res: the yardstick adds x + res in float64, the kernel
    normalises the fp32 sum it writes), da 6.8e-8, dgamma 5.7e-8, dbeta 4.0e-8; at (7, 2), where da is a cancellation, da 9.7e-9 - 5.8e-8;
    dgamma at d = 1 exactly zero."""
    x, res, dz, dsum, gamma, beta = data(rows, d)
    xd, dzd = dev(x, offset), dev(dz, offset)
    rd, dsd = (dev(res, offset), dev(dsum, offset)) if with_res else (None, None)
    gd, bd = (dev(gamma), dev(beta)) if affine else (None, None)
    out = dev(np.zeros_like(x), offset)
    if with_res:
        z, a = _native.ln_forward(xd, gd, bd, EPS, res=rd, out=out, sum_out=dev(np.zeros_like(x), offset))
    else:
        z, a = _native.ln_forward(xd, gd, bd, EPS, out=out), xd
    assert z is out
    da, dgamma, dbeta, ws = _native.ln_backward(a, dzd, gd, EPS, dsum=dsd)
    # the same call again, and with one parameter gradient wanted at a time: the same bits
    da2, dgamma2, dbeta2, _ = _native.ln_backward(a, dzd, gd, EPS, dsum=dsd, workspace=ws)
    da3, dgamma3, none3, _ = _native.ln_backward(a, dzd, gd, EPS, dsum=dsd, want_dbeta=False)
    da4, none4, dbeta4, _ = _native.ln_backward(a, dzd, gd, EPS, dsum=dsd, want_dgamma=False)
    da5, none5, none6, ws5 = _native.ln_backward(a, dzd, gd, EPS, dsum=dsd, want_dgamma=False, want_dbeta=False)
    torch.cuda.synchronize()
    assert torch.equal(xd, dev(x)) and torch.equal(dzd, dev(dz)), "the inputs are read only"
    want = yardstick(rows, d, with_res, affine)
    errs = {"z": rel_err(z.cpu().numpy(), want[0])}
    gerrs = grad_errs(d, da, dgamma, dbeta, want)
    print(f"({rows}, {d}) offset {offset} res {int(with_res)} affine {int(affine)}:", {k: f"{v:.2e}" for k, v in {**errs, **gerrs}.items()})
    if with_res:
        assert torch.equal(a, xd + rd), "sum is one fp32 add"
        assert torch.equal(rd, dev(res)) and torch.equal(dsd, dev(dsum))
    assert z.shape == xd.shape and da.shape == xd.shape and dgamma.shape == (d,) and dbeta.shape == (d,)
    assert none3 is None and none4 is None and none5 is None and none6 is None and ws5 is None
    for other in (da2, da3, da4, da5):
        assert torch.equal(da, other), "da does not depend on which parameter gradients are wanted, and two runs give the same bits"
    assert torch.equal(dgamma, dgamma2) and torch.equal(dgamma, dgamma3) and torch.equal(dbeta, dbeta2) and torch.equal(dbeta, dbeta4)
    if rows > 4:  # the constant row: z = beta exactly, da finite
        assert torch.equal(z[4], bd if affine else torch.zeros(d, device="cuda")), "a constant row gives z = beta"
    assert torch.isfinite(z).all() and torch.isfinite(da).all()
    assert all(e <= TOL for e in errs.values()), errs
    assert all(e <= TOL_GRAD for e in gerrs.values()), gerrs


@pytest.mark.parametrize("rows,d,offset", SHAPES, ids=IDS)
def test_in_place_sum_equals_out_of_place(rows, d, offset):
    x, res, _, _, gamma, beta = data(rows, d)
    gd, bd = dev(gamma), dev(beta)
    z, a = _native.ln_forward(dev(x, offset), gd, bd, EPS, res=dev(res, offset))
    over_x, over_res = dev(x, offset), dev(res, offset)
    z1, a1 = _native.ln_forward(over_x, gd, bd, EPS, res=dev(res, offset), sum_out=over_x)
    z2, a2 = _native.ln_forward(dev(x, offset), gd, bd, EPS, res=over_res, sum_out=over_res)
    torch.cuda.synchronize()
    assert a1 is over_x and a2 is over_res
    assert torch.equal(a1, a) and torch.equal(a2, a) and torch.equal(z1, z) and torch.equal(z2, z)


@pytest.mark.parametrize("rows,d,offset", [(130, 5, 0), (4099, 64, 0), (33, 260, 0)], ids=["130x5", "4099x64", "33x260"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_non_finite_row_stays_one_row(rows, d, offset, bad):
    x, res, dz, dsum, gamma, beta = data(rows, d)
    row = rows // 2 + 1
    xb = x.copy()
    xb[row, d // 3] = bad
    gd, bd = dev(gamma), dev(beta)
    z0, a0 = _native.ln_forward(dev(x), gd, bd, EPS, res=dev(res))
    da0 = _native.ln_backward(a0, dev(dz), gd, EPS, dsum=dev(dsum))[0]
    z, a = _native.ln_forward(dev(xb), gd, bd, EPS, res=dev(res))
    da, dgamma, dbeta, _ = _native.ln_backward(a, dev(dz), gd, EPS, dsum=dev(dsum))
    torch.cuda.synchronize()
    others = torch.arange(rows, device="cuda") != row
    assert not torch.isfinite(z[row]).any() and not torch.isfinite(da[row]).any(), "the whole row is non-finite"
    assert torch.equal(z[others], z0[others]) and torch.equal(da[others], da0[others]), "every other row is untouched"
    # the parameter gradients are poisoned as torch.nn.functional.layer_norm's are: dgamma everywhere (x^ of the row is non-finite),
    # dbeta = sum dz stays finite
    assert not torch.isfinite(dgamma).any() and torch.isfinite(dbeta).all()
    t = (dev(xb) + dev(res)).requires_grad_(True)
    w, b = gd.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    torch.nn.functional.layer_norm(t, (d,), w, b, EPS).backward(dev(dz))
    assert torch.equal(torch.isfinite(w.grad), torch.isfinite(dgamma)) and torch.equal(torch.isfinite(b.grad), torch.isfinite(dbeta))


def test_no_rows():
    for d in (5, 64):
        x = torch.zeros(0, d, device="cuda")
        g, b = torch.ones(d, device="cuda"), torch.zeros(d, device="cuda")
        z, a = _native.ln_forward(x, g, b, EPS, res=torch.zeros(0, d, device="cuda"))
        da, dgamma, dbeta, _ = _native.ln_backward(a, torch.zeros(0, d, device="cuda"), g, EPS)
        torch.cuda.synchronize()
        assert z.shape == (0, d) and a.shape == (0, d) and da.shape == (0, d)
        assert torch.equal(dgamma, torch.zeros(d, device="cuda")) and torch.equal(dbeta, torch.zeros(d, device="cuda"))
    y = _LayerNormFunction.apply(torch.zeros(2, 0, 8, device="cuda"), None, None, None, EPS)
    assert y.shape == (2, 0, 8)


def test_forward_under_stream_capture():
    rows, d = 4099, 64
    x, res, _, _, gamma, beta = data(rows, d)
    xd, rd, gd, bd = dev(x), dev(res), dev(gamma), dev(beta)
    want_z, want_a = _native.ln_forward(xd, gd, bd, EPS, res=rd)
    z, a = torch.zeros_like(xd), torch.zeros_like(xd)
    graph = torch.cuda.CUDAGraph()
    cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            _native.ln_forward(xd, gd, bd, EPS, res=rd, out=z, sum_out=a)
    cur.wait_stream(side)
    z.zero_()
    a.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(z, want_z) and torch.equal(a, want_a)


def test_the_autograd_function_with_both_outputs_used():
    """z and the sum both feed the loss, as in a transformer block: the one da comes back for x and for res."""
    rows, d = 1000, 16
    x, res, dz, dsum, gamma, beta = data(rows, d)
    t = [dev(v).view(2, rows // 2, d).requires_grad_(True) for v in (x, res)] + [dev(gamma).requires_grad_(True), dev(beta).requires_grad_(True)]
    z, a = _LayerNormFunction.apply(t[0], t[1], t[2], t[3], EPS)
    (z * dev(dz).view_as(z)).sum().backward(retain_graph=True)
    only_z = [v.grad.clone() for v in t]
    for v in t:
        v.grad = None
    ((z * dev(dz).view_as(z)).sum() + (a * dev(dsum).view_as(a)).sum()).backward()
    torch.cuda.synchronize()
    want = yardstick(rows, d, True, True)
    gerrs = grad_errs(d, t[0].grad.reshape(rows, d), t[2].grad, t[3].grad, want)
    no_dsum = ref.ln_backward(want[1], dz, EPS, gamma)[0]
    gerrs["da (sum unused)"] = rel_err(only_z[0].cpu().numpy().reshape(rows, d), no_dsum)
    print({k: f"{v:.2e}" for k, v in gerrs.items()})
    assert torch.equal(t[0].grad, t[1].grad) and torch.equal(only_z[0], only_z[1])
    assert all(e <= TOL_GRAD for e in gerrs.values()), gerrs
    # no affine: None for both parameters
    y = _LayerNormFunction.apply(dev(x), None, None, None, EPS)
    assert rel_err(y.cpu().numpy(), yardstick(rows, d, False, False)[0]) <= TOL


# ----------------------------------------------------------------------------------------------------------------- the layers


@functools.lru_cache(maxsize=None)
def knn_graph():
    A = healpix.healpix_graph(4)
    rows, cols = attention_ref.edges(A)
    return A, rows, cols


def _randomise(layer, seed):
    """Every parameter away from its special initial value (zero biases, unit gains), seeded."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in layer.named_parameters():
            r = torch.randn(p.shape, generator=gen)
            if name.endswith("bias"):
                p.copy_((0.3 * r).to(p.device))
            elif "layer_norm" in name or name.startswith("bn"):
                p.copy_((1.0 + 0.2 * r).to(p.device))
            else:
                p.copy_((r / np.sqrt(p.shape[-1])).to(p.device))


def _attention_block(dense, activation="relu", seed=3):
    A = knn_graph()[0]
    block = gnn_transformers.MultiHeadAttention(d_model=16, num_heads=2, activation=activation, dense=dense,
                                                sparse_A_indices=None if dense else A).cuda()
    _randomise(block, seed)
    return block


def _residual_block(axis=-1, seed=4):
    L = healpix.healpix_laplacian(4, mode="knn")
    kw = {"L": L, "K": 3, "use_bias": True, "activation": "elu", "device": "cuda:0"}
    block = GCNN_ResidualLayer("CHEBY", kw, activation="elu", use_bn=True, norm_type="layer_norm", bn_kwargs={"axis": axis})
    x = dev(np.random.default_rng(seed).standard_normal((2, L.shape[0], 8)))
    with torch.no_grad():
        block(x)  # builds the sub-layers and the norm modules
    _randomise(block, seed)
    return block, x, L


class _TorchLayerNormCalled(AssertionError):
    pass


def _boom(*a, **k):
    raise _TorchLayerNormCalled("torch.nn.functional.layer_norm was called")


def test_the_layers_no_longer_call_the_host_frameworks_layer_norm(monkeypatch):
    M = knn_graph()[0].shape[0]
    x = dev(np.random.default_rng(0).standard_normal((2, M, 16)))
    blocks = [_attention_block(False), _attention_block(True)]
    res_block, xr, _ = _residual_block()
    joint_block, _, _ = _residual_block(axis=(1, 2))
    monkeypatch.setattr(torch.nn.functional, "layer_norm", _boom)
    with pytest.raises(_TorchLayerNormCalled):  # the stub is in the path of the module it replaces
        torch.nn.LayerNorm(16).cuda()(x)
    for block in blocks:
        inp = x.clone().requires_grad_(True)
        block(inp).square().sum().backward()
        assert inp.grad is not None and all(p.grad is not None and torch.isfinite(p.grad).all() for p in block.parameters())
        with torch.no_grad():
            assert torch.isfinite(block(x)).all()
    for training in (True, False):
        inp = xr.clone().requires_grad_(True)
        res_block(inp, training=training).square().sum().backward()
        assert inp.grad is not None and all(p.grad is not None for p in res_block.parameters())
    with torch.no_grad():
        assert torch.isfinite(res_block(xr)).all()
    # the joint norm over pixels and channels is not the kernels': it must still reach torch
    with pytest.raises(_TorchLayerNormCalled):
        joint_block(xr)
    torch.cuda.synchronize()


def _block_composition(x, p, attention, act, d):
    """The transformer block as the torch ops it was before the kernels, on the parameters ``p`` in the dtype of x."""
    ln = torch.nn.functional.layer_norm
    x1 = ln(x, (d,), p["layer_norm1.weight"], p["layer_norm1.bias"], 1e-3)
    qkv = x1 @ p["wqkv.weight"].T + p["wqkv.bias"]
    att = x1 + attention(qkv[..., :d], qkv[..., d:2 * d], qkv[..., 2 * d:])
    y = ln(att, (d,), p["layer_norm2.weight"], p["layer_norm2.bias"], 1e-3)
    return act(y @ p["dense.weight"].T + p["dense.bias"]) + att


def _cheb_torch(Lt, x, kernel, K):
    """sum_k T_k(L~) x W_k with the layer's weight layout (row f K + k), dense L~, in the dtype of x."""
    t = [x, Lt @ x]
    for _ in range(2, K):
        t.append(2.0 * (Lt @ t[-1]) - t[-2])
    N, M, Fin = x.shape
    return torch.stack(t[:K], dim=-1).reshape(N, M, Fin * K) @ kernel


def _residual_composition(x, p, Lt, K, F):
    ln, elu = torch.nn.functional.layer_norm, torch.nn.functional.elu
    v = elu(_cheb_torch(Lt, x, p["layer1.kernel"], K) + p["layer1.bias"])
    v = ln(v, (F,), p["bn1.weight"], p["bn1.bias"], 1e-3)
    v = elu(_cheb_torch(Lt, v, p["layer2.kernel"], K) + p["layer2.bias"])
    v = ln(v, (F,), p["bn2.weight"], p["bn2.bias"], 1e-3)
    return elu(v + x)


def _cpu_grads(fn, x, params, g, dtype):
    p = {n: torch.tensor(a, dtype=dtype, requires_grad=True) for n, a in params.items()}
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    out = fn(xt, p)
    out.backward(torch.tensor(g, dtype=dtype))
    grads = {n: a.grad.numpy() for n, a in p.items()}
    grads["input"] = xt.grad.numpy()
    return out.detach().numpy(), grads


def _hold_to_ten_times_the_cpu(module, x, g, fn):
    """The rule of test_graph_transformer_end_to_end: the GPU's error against float64 is at most ten times the CPU fp32
    composition's, for the output and the gradient of every parameter and of the input."""
    inp = x.clone().requires_grad_(True)
    out = module(inp)
    out.backward(g)
    torch.cuda.synchronize()
    params = {n: p.detach().cpu().numpy() for n, p in module.named_parameters()}
    got = {n: p.grad.cpu().numpy() for n, p in module.named_parameters()}
    got["input"] = inp.grad.cpu().numpy()
    out64, g64 = _cpu_grads(fn, x.cpu().numpy(), params, g.cpu().numpy(), torch.float64)
    out32, g32 = _cpu_grads(fn, x.cpu().numpy(), params, g.cpu().numpy(), torch.float32)
    e_cpu, e_gpu = rel_err(out32, out64), rel_err(out.detach().cpu().numpy(), out64)
    print(f"output: cpu-fp32 {e_cpu:.2e} gpu {e_gpu:.2e}")
    failed = [] if e_gpu <= 10 * e_cpu else [("output", e_gpu, e_cpu)]
    for n in sorted(got):
        e_cpu, e_gpu = rel_err(g32[n], g64[n]), rel_err(got[n].reshape(g64[n].shape), g64[n])
        print(f"  d {n}: cpu-fp32 {e_cpu:.2e} gpu {e_gpu:.2e}")
        if not e_gpu <= 10 * e_cpu:
            failed.append((n, e_gpu, e_cpu))
    assert not failed, f"more than ten times the CPU fp32 error: {failed}"
    return out.detach()


@pytest.mark.parametrize("dense", [False, True], ids=["neighbours", "dense"])
def test_attention_block_against_the_composition_it_replaces(dense):
    _, rows, cols = knn_graph()
    M, d, heads = knn_graph()[0].shape[0], 16, 2
    block = _attention_block(dense, activation="elu")
    rng = np.random.default_rng(21)
    x, g = dev(rng.standard_normal((2, M, d))), dev(rng.standard_normal((2, M, d)))
    if dense:
        attention = lambda q, k, v: dense_attention_ref.attention_torch(q, k, v, heads)
    else:
        attention = lambda q, k, v: attention_ref.attention_torch(q, k, v, rows, cols, heads)
    _hold_to_ten_times_the_cpu(block, x, g, lambda t, p: _block_composition(t, p, attention, torch.nn.functional.elu, d))


def test_residual_block_against_the_composition_it_replaces():
    block, x, L = _residual_block()
    Lt, _ = orc.prepare_L(L)
    K, F = 3, 8
    # the torch restatement of the convolution is the oracle's
    k1 = block.layer1.kernel.detach().cpu().numpy().astype(np.float64)
    x64 = x.cpu().numpy().astype(np.float64)
    dense64 = torch.tensor(sparse.csr_matrix(Lt).toarray(), dtype=torch.float64)
    assert rel_err(_cheb_torch(dense64, torch.tensor(x64), torch.tensor(k1), K).numpy(), orc.chebyshev_forward(Lt, x64, k1, K)) <= 1e-12
    g = dev(np.random.default_rng(22).standard_normal(tuple(x.shape)))
    block.train()

    def fn(t, p):
        p = dict(p)
        for n in ("layer1.bias", "layer2.bias"):
            p[n] = p[n].reshape(-1)
        return _residual_composition(t, p, dense64.to(t.dtype), K, F)

    _hold_to_ten_times_the_cpu(_Named(block, training=True), x, g, fn)


class _Named:
    """A residual block called with ``training=...`` that still answers ``named_parameters``."""

    def __init__(self, block, training):
        self.block, self.training = block, training

    def __call__(self, t):
        return self.block(t, training=self.training)

    def named_parameters(self):
        return self.block.named_parameters()


@pytest.mark.parametrize("activation", ["relu", "elu", "tanh", torch.nn.functional.softplus, None],
                         ids=["relu", "elu", "tanh", "callable", "none"])
@pytest.mark.parametrize("dense", [False, True], ids=["neighbours", "dense"])
def test_inference_tail_on_the_epilogue_equals_the_autograd_path(dense, activation, monkeypatch):
    block = _attention_block(dense, activation=activation)
    M = knn_graph()[0].shape[0]
    x = dev(np.random.default_rng(5).standard_normal((2, M, 16)))
    want = block(x.clone().requires_grad_(True)).detach()  # autograd on: the tail is the host framework's
    calls = []
    real = _native.residual_epilogue
    monkeypatch.setattr(_native, "residual_epilogue", lambda *a, **k: (calls.append(a[2:]), real(*a, **k))[1])
    with torch.no_grad():
        got = block(x)
    torch.cuda.synchronize()
    has_code = activation is None or isinstance(activation, str)
    assert len(calls) == (1 if has_code else 0), "act(dense(y)) + att in one pass exactly when the activation has a code"
    if has_code:
        assert calls[0][0] == 1.0 and calls[0][2] is True
    torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-6)
