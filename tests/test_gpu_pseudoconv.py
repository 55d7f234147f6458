"""GPU tests of the pseudo-convolutions on the patch GEMM (csrc/patch_gemm.hip): the kernels against the float64 yardstick
(tests/pseudoconv_ref.py) on every path the code takes, the two layers against the oracle and the yardstick, their state across
calls, and the reference's autoencoder.  Error measure: ``helpers.rel_err``; bounds: 1e-5 for Y in "fp32" and "bf16x6", 2e-5 for
Y in "bf16x3" (only where the contraction is at least 16 long, the rule of gnn_layers.py), 2e-5 for dX, dW and db."""

import functools

import numpy as np
import pytest
import torch

import pseudoconv_ref as ref
from deepsphere import _native, healpy_layers
from deepsphere.healpy_networks import HealpyGCNN
from helpers import offset_view, rel_err
from oracle import cheb_oracle as orc

pytestmark = pytest.mark.gpu

TOL, TOL_BF16X3, TOL_GRAD = 1e-5, 2e-5, 2e-5
PRECS = {"fp32": _native.PREC_FP32, "bf16x6": _native.PREC_BF16X6, "bf16x3": _native.PREC_BF16X3}
ACTS = {"none": _native.ACT_NONE, "relu": _native.ACT_RELU, "elu": _native.ACT_ELU, "sigmoid": _native.ACT_SIGMOID, "tanh": _native.ACT_TANH}

# (R, Kd, C, P, floats off 16-byte alignment)
SHAPES = [
    (1, 4, 1, 1, 0),          # one row, one column, Fin = 1 at p = 1
    (3, 64, 5, 5, 0),         # p = 2, Fin = 4, odd C
    (130, 24, 10, 10, 0),     # the shape of test_pseudo_convolutions_against_the_oracle, ragged last wave
    (4099, 256, 64, 64, 0),   # 64 -> 64 at p = 1, several workgroups, row tail
    (257, 1024, 32, 32, 0),   # Kd over many LDS chunks
    (64, 320, 96, 96, 0),     # p = 3, Fin = 5, three column blocks
    (515, 20, 12, 12, 1),     # scalar path through misaligned maps
    (1, 1, 4, 1, 0),          # transpose, Fin = Fout = 1
    (130, 6, 40, 10, 0),      # transpose of the existing test's shape, periodic bias
    (4099, 64, 256, 64, 0),   # 64 -> 64 transpose at p = 1
    (33, 70, 80, 5, 0),       # Kd not a multiple of 4, p = 2
    (257, 16, 192, 3, 0),     # p = 3, period 3 across vector boundaries
    (515, 5, 28, 7, 1),       # misaligned transpose
]
MORE_ACTS = {(130, 24, 10, 10, 0), (130, 6, 40, 10, 0)}  # tanh and sigmoid as well


@functools.lru_cache(maxsize=None)
def _case(shape):
    R, Kd, C, P, _ = shape
    return ref.make_data(R, Kd, C, P, seed=1)


@functools.lru_cache(maxsize=None)
def _case_ref(shape, act):
    X, W, b, dY = _case(shape)
    P = shape[3]
    Y = ref.patch_forward(X, W, b, P, act)
    return (Y,) + ref.patch_backward(X, W, Y, dY, P, act)


def _dev(a, off=0):
    return offset_view(a, off) if off else torch.as_tensor(a, device="cuda")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_against_the_yardstick(shape):
    """Largest measured on an MI355X, over all shapes and activations: Y fp32 1.2e-6, bf16x6 9.3e-7, bf16x3 1.83e-5 (at
    (130, 24, 10, 10) with tanh, whose outputs are bounded by 1 while its pre-activations reach 3: 7e-6 of max|z| becomes 1.8e-5 of
    max|y|; 7.1e-6 at most with the other activations); dX fp32 6.1e-7, bf16x6 5.9e-7, bf16x3 7.0e-6; dW 2.7e-6; db 1.7e-7."""
    R, Kd, C, P, off = shape
    X, W, b, dY = _case(shape)
    x, w, bias, dy = _dev(X, off), _dev(W), _dev(b), _dev(dY, off)
    keep = [t.clone() for t in (x, w, bias, dy)]
    acts = ["none", "relu", "elu"] + (["sigmoid", "tanh"] if shape in MORE_ACTS else [])
    for act in acts:
        Yr, dXr, dWr, dbr = _case_ref(shape, act)
        for prec, code in PRECS.items():
            if prec == "bf16x3" and Kd < 16:
                continue
            out = _dev(np.zeros((R, C), np.float32), off)
            y = _native.patch_gemm(x, w, bias, P, act=ACTS[act], precision=code, out=out)
            assert y is out
            e = rel_err(y.cpu().numpy(), Yr)
            print(f"{shape} {act} {prec}: y {e:.2e}")
            assert e <= (TOL_BF16X3 if prec == "bf16x3" else TOL), (shape, act, prec, e)
            if act == "none":  # no bias is a zero bias
                y0 = _native.patch_gemm(x, w, torch.zeros_like(bias), P, act=ACTS[act], precision=code)
                assert torch.equal(_native.patch_gemm(x, w, None, P, act=ACTS[act], precision=code), y0)
        # the backward on the stored fp32-equivalent output
        y = _native.patch_gemm(x, w, bias, P, act=ACTS[act], precision=_native.PREC_BF16X6, out=_dev(np.zeros((R, C), np.float32), off))
        ya = y if act != "none" else None
        dz, db, ws = _native.patch_epilogue_backward(ya, dy, P, act=ACTS[act], out=_dev(np.zeros((R, C), np.float32), off))
        dz2, db2, _ = _native.patch_epilogue_backward(ya, dy, P, act=ACTS[act], workspace=ws.fill_(255))
        assert torch.equal(dz, dz2) and torch.equal(db, db2), "the same call twice gives the same bits"
        dz3, none, _ = _native.patch_epilogue_backward(ya, dy, P, act=ACTS[act], want_dbias=False)
        assert none is None and torch.equal(dz3, dz), "without a bias gradient dz is the same"
        dyc = _dev(dY, off)
        dz4, db4, _ = _native.patch_epilogue_backward(ya, dyc, P, act=ACTS[act], out=dyc)
        assert dz4 is dyc and torch.equal(dz4, dz) and torch.equal(db4, db), "in place"
        e = rel_err(db.cpu().numpy(), dbr)
        print(f"{shape} {act}: db {e:.2e}")
        assert e <= TOL_GRAD, (shape, act, "db", e)
        dw, _ = _native.cheb_wgrad([x.view(1, R, Kd)], dz.view(1, R, C))
        e = rel_err(dw.cpu().numpy(), dWr)
        print(f"{shape} {act}: dw {e:.2e}")
        assert e <= TOL_GRAD, (shape, act, "dw", e)
        wt = w.t().contiguous()
        for prec, code in PRECS.items():
            if prec == "bf16x3" and C < 16:
                continue
            dx = _native.patch_gemm(dz, wt, None, 1, precision=code)
            e = rel_err(dx.cpu().numpy(), dXr)
            print(f"{shape} {act} {prec}: dx {e:.2e}")
            assert e <= TOL_GRAD, (shape, act, prec, "dx", e)
    for t, k in zip((x, w, bias, dy), keep):
        assert torch.equal(t, k), "the inputs are unchanged"


# ---- the layers -----------------------------------------------------------------------------------------------------------------

M_PIX = 768


def _layer_problem(layer, x):
    """-> X, W, bias, P and the map shape of the layer's GEMM on its own weights (numpy)."""
    weight = layer.filter.weight.detach().cpu().numpy()
    bias = None if layer.filter.bias is None else layer.filter.bias.detach().cpu().numpy()
    N, M, Fin = x.shape
    g = layer.filter_size
    if isinstance(layer, healpy_layers.HealpyPseudoConv_Transpose):
        return x.reshape(N * M, Fin), ref.conv_transpose_image(weight), bias, (N, M * g, layer.Fout)
    return x.reshape(N * M // g, g * Fin), ref.conv_image(weight), bias, (N, M // g, layer.Fout)


def _check_layer(cls, p, Fin, Fout, activation, use_bias=True, precision="auto"):
    rng = np.random.default_rng([p, Fin, Fout])
    x = rng.standard_normal((2, M_PIX, Fin)).astype(np.float32)
    layer = cls(p, Fout, activation=activation, use_bias=use_bias, precision=precision,
                bias_initializer=lambda b: torch.nn.init.normal_(b, std=0.3)).cuda()
    xt = torch.as_tensor(x, device="cuda").requires_grad_(True)
    y = layer(xt)
    transpose = cls is healpy_layers.HealpyPseudoConv_Transpose
    g = layer.filter_size
    X, W, bias, shape = _layer_problem(layer, x)
    assert tuple(y.shape) == shape and (layer.filter.bias is not None) == use_bias
    # forward: the oracle's restatement of the Keras layer, then the activation in float64
    kernel = np.transpose(layer.filter.weight.detach().cpu().numpy().astype(np.float64), (2, 1, 0))
    lin = (orc.healpy_pseudo_conv_transpose if transpose else orc.healpy_pseudo_conv)(x.astype(np.float64), kernel, bias, p)
    tl = torch.tensor(lin, requires_grad=True)
    ta = {None: tl, "elu": torch.nn.functional.elu(tl), "gelu": torch.nn.functional.gelu(tl)}[activation]
    dy = rng.standard_normal(shape).astype(np.float32)
    ta.backward(torch.tensor(dy.astype(np.float64)))
    tol_y = TOL_BF16X3 if precision == "bf16x3" else TOL
    errs = {"y": (rel_err(y.detach().cpu().numpy(), ta.detach().numpy()), tol_y)}
    with torch.no_grad():
        errs["y no-grad"] = (rel_err(layer(xt.detach()).cpu().numpy(), ta.detach().numpy()), tol_y)
    y.backward(torch.as_tensor(dy, device="cuda"))
    # gradients: the yardstick on the pre-activation gradient (the activation's own derivative from torch float64)
    C = W.shape[1]
    dX, dW, db = ref.patch_backward(X, W, lin.reshape(-1, C), tl.grad.numpy().reshape(-1, C), Fout, None)
    dweight = ref.conv_transpose_image_inverse(dW, Fout, g) if transpose else ref.conv_image_inverse(dW, Fin, g)
    errs["dx"] = (rel_err(xt.grad.cpu().numpy(), dX.reshape(x.shape)), TOL_GRAD)
    errs["dweight"] = (rel_err(layer.filter.weight.grad.cpu().numpy(), dweight), TOL_GRAD)
    if use_bias:
        errs["dbias"] = (rel_err(layer.filter.bias.grad.cpu().numpy(), db), TOL_GRAD)
    print(cls.__name__, p, Fin, Fout, activation, use_bias, precision, {k: f"{v[0]:.2e}" for k, v in errs.items()})
    for name, (e, tol) in errs.items():
        assert e <= tol, (name, e, tol)


@pytest.mark.parametrize("activation", [None, "elu", "gelu"])
@pytest.mark.parametrize("Fin,Fout", [(1, 8), (6, 10), (64, 64)])
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("cls", [healpy_layers.HealpyPseudoConv, healpy_layers.HealpyPseudoConv_Transpose], ids=["conv", "transpose"])
def test_layers_forward_and_gradients(cls, p, Fin, Fout, activation):
    """Largest measured on an MI355X: y 1.1e-6 (Kd = 1024), dx 1.4e-6, dweight 1.8e-6, dbias 2.7e-7."""
    _check_layer(cls, p, Fin, Fout, activation)


@pytest.mark.parametrize("cls", [healpy_layers.HealpyPseudoConv, healpy_layers.HealpyPseudoConv_Transpose], ids=["conv", "transpose"])
def test_layers_without_bias_and_on_the_three_term_split(cls):
    """Largest measured on an MI355X with "bf16x3" at 64 -> 64: y 4.7e-6, dx 6.7e-6, dweight 2.5e-6, dbias 2.9e-6."""
    _check_layer(cls, 1, 6, 10, "elu", use_bias=False)
    _check_layer(cls, 1, 6, 10, None, use_bias=False)
    _check_layer(cls, 1, 64, 64, "elu", precision="bf16x3")
    # "auto" keeps the library GEMM at these shapes (the layers' shape rule); by name the kernel runs them
    _check_layer(cls, 1, 64, 64, "elu", precision="bf16x6")
    _check_layer(cls, 2, 64, 64, None, precision="fp32")


def test_shape_rule_of_the_default_arithmetic(monkeypatch):
    """precision="auto": the kernel where Kd <= 64 and C <= 256, the library GEMM composition beyond; a precision asked for by
    name runs the kernel at every shape.  Both give the same map (to the tolerance of the forward)."""
    calls = []
    real = _native.patch_gemm
    monkeypatch.setattr(_native, "patch_gemm", lambda *a, **k: (calls.append(tuple(a[0].shape) + (int(a[1].shape[1]),)), real(*a, **k))[1])
    x = torch.as_tensor(np.random.default_rng(2).standard_normal((1, 192, 64)).astype(np.float32), device="cuda")
    cases = [(healpy_layers.HealpyPseudoConv, 1, 64, "auto", False),        # Kd 256
             (healpy_layers.HealpyPseudoConv, 1, 64, "bf16x6", True),
             (healpy_layers.HealpyPseudoConv_Transpose, 1, 64, "auto", True),   # Kd 64, C 256
             (healpy_layers.HealpyPseudoConv_Transpose, 2, 64, "auto", False),  # C 1024
             (healpy_layers.HealpyPseudoConv_Transpose, 2, 64, "fp32", True),
             (healpy_layers.HealpyPseudoConv_Transpose, 1, 65, "auto", False)]  # C 260
    for cls, p, Fout, precision, on_kernel in cases:
        layer = cls(p, Fout, activation="elu", precision=precision).cuda()
        del calls[:]
        with torch.no_grad():
            y = layer(x)
        assert bool(calls) == on_kernel, (cls.__name__, p, Fout, precision, calls)
        X, W, bias, shape = _layer_problem(layer, x.cpu().numpy())
        assert rel_err(y.cpu().numpy(), ref.patch_forward(X, W, bias, Fout, "elu").reshape(shape)) <= TOL
    small = healpy_layers.HealpyPseudoConv(1, 32, precision="auto").cuda()  # Kd 64, C 32: the largest reduction under the rule
    del calls[:]
    with torch.no_grad():
        small(x[..., :16])
    assert calls == [(48, 64, 32)]


# ---- state across calls ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", [healpy_layers.HealpyPseudoConv, healpy_layers.HealpyPseudoConv_Transpose], ids=["conv", "transpose"])
def test_state_across_calls(cls):
    rng = np.random.default_rng(11)
    x = torch.as_tensor(rng.standard_normal((3, 192, 6)).astype(np.float32), device="cuda")
    layer = cls(1, 10, activation="elu", bias_initializer=lambda b: torch.nn.init.normal_(b, std=0.3)).cuda()

    def want(xs):
        X, W, bias, shape = _layer_problem(layer, xs.cpu().numpy())
        return ref.patch_forward(X, W, bias, 10, "elu").reshape(shape)

    with torch.no_grad():
        y0 = layer(x)
        assert rel_err(y0.cpu().numpy(), want(x)) <= TOL
        layer.filter.weight.mul_(-1.5)  # in place: the second forward follows the new weights
        layer.filter.bias.add_(0.25)
        y1 = layer(x)
        assert rel_err(y1.cpu().numpy(), want(x)) <= TOL and rel_err(y1.cpu().numpy(), y0.cpu().numpy()) > 0.1
        layer.train()
        yt = layer(x)
        layer.eval()
        assert torch.equal(yt, y1) and torch.equal(layer(x), y1), ".train() / .eval() make no difference"
        for n in (1, 3, 1):  # batch 1, then 3, then 1 on one instance
            assert torch.equal(layer(x[:n]), y1[:n])
    # with autograd the same bits as without
    assert torch.equal(layer(x.clone().requires_grad_(True)).detach(), y1)
    # one forward captured on a single stream, replayed on new contents
    static = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        layer(static)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out = layer(static)
    x2 = torch.as_tensor(rng.standard_normal(tuple(x.shape)).astype(np.float32), device="cuda")
    static.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        assert torch.equal(out, layer(x2)), "the replay equals the eager forward bit for bit"


# ---- the reference's autoencoder (examples/generative_models.ipynb) ---------------------------------------------------------------

def test_autoencoder_forward_and_backward():
    torch.manual_seed(0)
    enc = [healpy_layers.HealpyPseudoConv(p=1, Fout=F, activation="elu") for F in (4, 8, 16)]
    dec = [healpy_layers.HealpyPseudoConv_Transpose(p=1, Fout=F, activation=a) for F, a in ((16, "elu"), (16, "elu"), (1, "linear"))]
    model = HealpyGCNN(nside=8, indices=np.arange(768), layers=enc + dec)
    x = torch.as_tensor(np.random.default_rng(7).standard_normal((3, 768, 1)).astype(np.float32))
    model(x)  # builds the filters
    with torch.no_grad():
        for layer in enc + dec:
            layer.filter.bias.normal_(std=0.3)
        want = model(x).numpy()
    model.cuda()
    y = model(x.cuda())
    assert tuple(y.shape) == (3, 768, 1)
    err = rel_err(y.detach().cpu().numpy(), want)
    print(f"autoencoder on the GPU vs the CPU run of the same weights: {err:.2e}")
    assert err <= 1e-5
    ((y - x.cuda()) ** 2).mean().backward()
    params = list(model.parameters())
    assert len(params) == 12
    for prm in params:
        assert prm.grad is not None and torch.isfinite(prm.grad).all() and prm.grad.abs().max() > 0
