"""GPU tests of the weight basis-change kernel (``dsph_basis_change``) and of ``Bernstein`` / ``HealpyBernstein`` on it
(``pytest -m gpu``).

Reference: tests/bernstein_ref.py, the reference's op sequence restated in float64 ON THE LAYER'S OWN fp32 L~, so only the
arithmetic is compared.

Kernel bound (derived): an output is one fp32 fma chain over i = 0 .. Kp - 1.  The Kp roundings of the chain each are at most
2^-24 of a partial sum no larger than S = sum_i |c(i,j)| |w_i| (times (1 + 2^-24)^Kp), one more unit covers that factor:
    |err| <= (Kp + 1) 2^-24 sum_i |c(i,j)| |w_i|     per element.
Layer tolerances are the project's own (fractions of max|y| or of the gradient's maximum): 2e-6 for the fp32-equivalent
arithmetics ("fp32", "bf16x6", "f16x3": TOL_FP32_EQUIV), 2e-5 for the three-term bf16 split ("bf16x3", and "auto" where it
resolves to it: Fin >= 16 and no chain of passes; where "auto" resolves to "bf16x6" it is held to that one's 2e-6), 1e-5 for the
exact-fp32 backward (TOL), 2e-5 for the split weight gradient (TOL_QWGRAD).

Measured on an MI355X (every figure is printed by the tests; smallest - largest over ``FORWARD_CASES``, fractions of max|y| or max|gradient|):
    forward, 16 or more input channels:  "fp32", "bf16x6", "f16x3" 1.9e-7 - 8.3e-7;  "bf16x3" and "auto" 4.2e-6 - 1.14e-5
    forward, fewer input channels:       "fp32", "bf16x6", "f16x3", "auto" 6.6e-8 - 2.2e-7;  "bf16x3" 2.3e-6 - 1.6e-5 (reported only)
    backward "fp32", nside 4:            dx 2.5e-7 (K = 2), 4.6e-7 (K = 5);  dkernel 1.7e-7, 2.7e-7
    backward "auto", nside 16, K = 5:    dx 6.6e-6, dkernel 4.5e-6 (the split weight gradient); "fp32" there: 8.0e-7, 2.9e-7
No required shape exceeds 2e-5 under "bf16x3", so "auto" resolves for Bernstein as it does for Chebyshev.
"""

import functools

import numpy as np
import pytest
import torch

import bernstein_ref as ref
from deepsphere import _native, healpix, utils
from deepsphere.gnn_layers import Bernstein, Chebyshev, bernstein_to_chebyshev, resolve_precision
from deepsphere.healpy_layers import HealpyBernstein, HealpyPool
from deepsphere.healpy_networks import HealpyGCNN
from helpers import rel_err

pytestmark = pytest.mark.gpu

TOL_FP32_EQUIV = 2e-6
TOL_BF16X3 = 2e-5
TOL = 1e-5
TOL_QWGRAD = 2e-5


# ---------------------------------------------------------------------------------------------------------------- the kernel

def _kernel_inputs(Fin, Fout, Kp):
    rng = np.random.default_rng(1000 * Fin + 10 * Fout + Kp)
    return (rng.standard_normal((Fin * Kp, Fout)).astype(np.float32), rng.standard_normal((Kp, Kp)).astype(np.float32))


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("Fin,Fout,Kp", [(1, 1, 2), (3, 5, 3), (7, 3, 5), (16, 32, 6), (64, 64, 6), (5, 130, 11)])
def test_basis_change_kernel(Fin, Fout, Kp, transpose):
    w, c = _kernel_inputs(Fin, Fout, Kp)
    got = _native.basis_change(torch.as_tensor(w).cuda(), torch.as_tensor(c).cuda(), transpose=transpose)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    cm = (c.T if transpose else c).astype(np.float64)          # cm[i, j] = c(i, j)
    w3 = w.astype(np.float64).reshape(Fin, Kp, Fout)
    want = np.einsum("ij,fio->fjo", cm, w3).reshape(Fin * Kp, Fout)
    bound = (Kp + 1) * 2.0**-24 * np.einsum("ij,fio->fjo", np.abs(cm), np.abs(w3)).reshape(Fin * Kp, Fout)
    err = np.abs(got - want)
    print(f"{Fin} x {Kp} -> {Fout} transpose {int(transpose)}: worst err / bound {np.max(err / bound):.3f}")
    assert got.dtype == np.float32 and got.shape == w.shape and np.all(err <= bound)


def test_basis_change_into_a_given_buffer_and_twice_the_same_bits():
    w, c = (torch.as_tensor(a).cuda() for a in _kernel_inputs(16, 32, 6))
    out = torch.full_like(w, float("nan"))
    assert _native.basis_change(w, c, out=out) is out
    assert torch.equal(out, _native.basis_change(w, c)) and not torch.equal(out, _native.basis_change(w, c, transpose=True))
    with pytest.raises(ValueError):
        _native.basis_change(w, c, out=w)                       # in place: refused by the library
    with pytest.raises(ValueError):
        _native.basis_change(w, c[:5, :5].contiguous())         # 96 rows are no multiple of 5


def test_basis_change_bad_arguments_are_reported():
    lib = _native.lib()
    w, c = (torch.as_tensor(a).cuda() for a in _kernel_inputs(4, 8, 3))
    out = torch.empty_like(w)
    stream = _native._stream_ptr(w.device)
    p = _native._ptr

    def call(wp, cp, op, Kp):
        return lib.dsph_basis_change(wp, cp, op, 4, 8, Kp, 0, w.device.index, stream)

    for what, rc in (("w_out == w", call(p(w), p(c), p(w), 3)), ("Kp = 0", call(p(w), p(c), p(out), 0)),
                     ("Kp = 65", call(p(w), p(c), p(out), 65)), ("w NULL", call(p(None), p(c), p(out), 3)),
                     ("coeff NULL", call(p(w), p(None), p(out), 3)), ("w_out NULL", call(p(w), p(c), p(None), 3))):
        assert rc == -1, what                                   # DSPH_E_BADARG
        assert "basis_change" in _native.last_error()
    assert call(p(w), p(c), p(out), 3) == 0                     # and the library still works
    torch.cuda.synchronize()
    assert torch.equal(out, _native.basis_change(w, c))


def test_basis_change_under_stream_capture():
    w, c = (torch.as_tensor(a).cuda() for a in _kernel_inputs(16, 32, 6))
    want = _native.basis_change(w, c)
    out = torch.zeros_like(w)
    graph = torch.cuda.CUDAGraph()
    cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            _native.basis_change(w, c, out=out)
    cur.wait_stream(side)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


# ----------------------------------------------------------------------------------------------------------------- the layer

@functools.lru_cache(maxsize=None)
def graph(name):
    """-> (ELL columns, ELL values, the same fp32 L~ as a float64 CSR matrix)."""
    if name == "dense3":       # the shape of the reference's own layer test: a dense symmetric 3 x 3 matrix
        A = np.random.default_rng(11).standard_normal((3, 3))
        L = A @ A.T
    elif name == "n4":
        L = healpix.healpix_laplacian(4)
    elif name == "n8cap":      # 260 pixels, ragged rows
        L = healpix.healpix_laplacian(8, indices=healpix.cap_indices(8))
    elif name == "n16":        # 3,072 pixels on the 8-neighbour stencil: the fused tiles
        L = healpix.healpix_laplacian(16, mode="grid")
    Lt, _ = utils.prepare_L(L, scale=0.75)
    cols, vals = utils.csr_to_ell(Lt)
    return cols, vals, ref.csr(cols, vals)


@functools.lru_cache(maxsize=None)
def data(name, N, Fin, Fout, K):
    """x, dy, kernel (float32 numpy; the kernel at the default initialiser's scale); shared, never written."""
    M = graph(name)[0].shape[0]
    rng = np.random.default_rng(7 * Fin + Fout + 100 * K)
    x = rng.standard_normal((N, M, Fin)).astype(np.float32)
    dy = rng.standard_normal((N, M, Fout)).astype(np.float32)
    kernel = (rng.standard_normal(((K + 1) * Fin, Fout)) * np.sqrt(6.0 / (Fin + Fout))).astype(np.float32)
    return x, dy, kernel


@functools.lru_cache(maxsize=None)
def oracle_forward(name, N, Fin, Fout, K):
    x, _, kernel = data(name, N, Fin, Fout, K)
    return ref.forward(graph(name)[2], x, kernel, K)


def make(name, K, Fin, kernel, cls=Bernstein, **kw):
    cols, vals, _ = graph(name)
    layer = cls.from_prepared_ell(cols, vals, K, Fout=int(kernel.shape[1]), **kw)
    layer.build((1, cols.shape[0], Fin))
    with torch.no_grad():
        layer.kernel.copy_(torch.as_tensor(kernel))
    return layer


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda()


FORWARD_CASES = ([("dense3", 4, 7, 3, 5)]
                 + [(g, K, Fin, Fout, 2) for g in ("n4", "n8cap", "n16") for K in (1, 2, 5) for Fin, Fout in ((1, 16), (16, 32), (64, 64))]
                 + [("n8cap", 9, 16, 16, 2)])   # ten terms: the route of layers with more than nine


@pytest.mark.parametrize("name,K,Fin,Fout,N", FORWARD_CASES)
def test_forward_parity(name, K, Fin, Fout, N):
    x, _, kernel = data(name, N, Fin, Fout, K)
    want = oracle_forward(name, N, Fin, Fout, K)
    xd = dev(x)
    missed = []
    for prec in ("fp32", "bf16x6", "f16x3", "bf16x3", "auto"):
        layer = make(name, K, Fin, kernel, precision=prec)
        with torch.no_grad():
            y = layer(xd)
        torch.cuda.synchronize()
        err = rel_err(y.cpu().numpy(), want)
        resolved = resolve_precision(prec, Fin, K + 1, layer._chained())
        tol = TOL_BF16X3 if resolved == "bf16x3" else TOL_FP32_EQUIV
        held = not (prec == "bf16x3" and Fin < 16)   # (the three-term split below 16 channels: nothing averages out; not a default)
        print(f"{name} K {K} {Fin}->{Fout} {prec} ({resolved}): {err:.2e}{'' if held else ' (reported only)'}")
        assert tuple(y.shape) == (N, x.shape[1], Fout) and np.isfinite(err)
        if held and not err < tol:
            missed.append((prec, resolved, err, tol))
    assert not missed, missed


@pytest.mark.parametrize("epilogue", [False, True])
def test_same_bits_as_a_chebyshev_layer_on_the_transformed_weights(epilogue):
    name, K, Fin, Fout, N = "n16", 5, 16, 32, 2
    x, _, kernel = data(name, N, Fin, Fout, K)
    kw = dict(use_bn=True, use_bias=True, activation="relu") if epilogue else {}
    bern = make(name, K, Fin, kernel, **kw)
    C = torch.as_tensor(bernstein_to_chebyshev(K).astype(np.float32)).cuda()
    cheb = make(name, K + 1, Fin, _native.basis_change(dev(kernel), C).cpu().numpy(), cls=Chebyshev, **kw)
    assert torch.equal(bern._coeff_on(C.device), C)
    if epilogue:
        rng = np.random.default_rng(5)
        mean, var, bias = rng.standard_normal(Fout), rng.random(Fout) + 0.5, rng.standard_normal((1, 1, Fout))
        with torch.no_grad():
            for layer in (bern, cheb):
                layer.bn.running_mean.copy_(torch.as_tensor(mean))
                layer.bn.running_var.copy_(torch.as_tensor(var))
                layer.bias.copy_(torch.as_tensor(bias))
    with torch.no_grad():
        yb, yc = bern(dev(x)), cheb(dev(x))
    torch.cuda.synchronize()
    assert bern._prec_code() == cheb._prec_code() and torch.equal(yb, yc)
    if epilogue:   # and the values are the oracle's through BN -> bias -> ReLU
        s = 1.0 / np.sqrt(var + 1e-5)
        want = np.maximum((oracle_forward(name, N, Fin, Fout, K) - mean) * s + bias, 0.0)
        assert rel_err(yb.cpu().numpy(), want) < TOL_BF16X3


def _backward(name, K, Fin, Fout, N, precision):
    x, dy, kernel = data(name, N, Fin, Fout, K)
    Lt = graph(name)[2]
    layer = make(name, K, Fin, kernel, precision=precision)
    xd = dev(x).requires_grad_(True)
    y = layer(xd)
    y.backward(dev(dy))
    torch.cuda.synchronize()
    ex = rel_err(xd.grad.cpu().numpy(), ref.grad_x(Lt, kernel, K, dy))
    ek = rel_err(layer.kernel.grad.cpu().numpy(), ref.grad_w(Lt, x, K, dy))
    ey = rel_err(y.detach().cpu().numpy(), oracle_forward(name, N, Fin, Fout, K))
    print(f"{name} K {K} {Fin}->{Fout} {precision}: dx {ex:.2e} dkernel {ek:.2e} (y {ey:.2e})")
    assert tuple(xd.grad.shape) == x.shape and tuple(layer.kernel.grad.shape) == kernel.shape
    return ex, ek


@pytest.mark.parametrize("K", [2, 5])
def test_backward_exact_fp32(K):
    ex, ek = _backward("n4", K, 16, 16, 2, "fp32")
    assert ex < TOL and ek < TOL


def test_backward_default_arithmetic_with_the_split_weight_gradient():
    ex, ek = _backward("n16", 5, 16, 32, 2, "auto")   # N * M = 6,144 pixels >= WGRAD_SPLIT_MIN_PIXELS
    assert ex < TOL_QWGRAD and ek < TOL_QWGRAD


def test_training_step_with_bias_and_batch_norm():
    name, K, Fin, Fout, N = "n4", 5, 16, 16, 2
    x, dy, kernel = data(name, N, Fin, Fout, K)
    layer = make(name, K, Fin, kernel, use_bias=True, use_bn=True, activation="relu")
    before = layer.bn.running_mean.clone()
    xd = dev(x).requires_grad_(True)
    y = layer(xd, training=True)
    (y * dev(dy)).sum().backward()
    torch.cuda.synchronize()
    assert tuple(y.shape) == (N, 192, Fout)
    for g, shape in ((xd.grad, x.shape), (layer.kernel.grad, kernel.shape), (layer.bias.grad, (1, 1, Fout))):
        assert tuple(g.shape) == tuple(shape) and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    assert not torch.equal(before, layer.bn.running_mean)     # batch statistics were used and the moving ones updated


def test_transformed_weights_are_cached_and_follow_the_kernel():
    name, K, Fin, Fout, N = "n8cap", 5, 16, 32, 2
    x, _, kernel = data(name, N, Fin, Fout, K)
    Lt = graph(name)[2]
    layer = make(name, K, Fin, kernel)
    xd = dev(x)
    with torch.no_grad():
        ys = [layer(xd) for _ in range(3)]
    assert layer._basis_image["count"] == 1 and torch.equal(ys[0], ys[2])
    buf = layer._basis_image["kernel"].data_ptr()
    with torch.no_grad():
        layer.kernel.mul_(0.5)
        y = layer(xd)
        layer(xd)
    torch.cuda.synchronize()
    assert layer._basis_image["count"] == 2 and layer._basis_image["kernel"].data_ptr() == buf
    assert rel_err(y.cpu().numpy(), ref.forward(Lt, x, 0.5 * kernel.astype(np.float64), K)) < TOL_BF16X3
    assert rel_err(ys[0].cpu().numpy(), oracle_forward(name, N, Fin, Fout, K)) < TOL_BF16X3
    assert "_coeff" not in layer.state_dict() and set(layer.state_dict()) == {"kernel"}


def test_graph_replay_gives_the_plain_forward():
    name, K, Fin, Fout, N = "n16", 5, 16, 32, 2
    x, _, kernel = data(name, N, Fin, Fout, K)
    plain, captured = make(name, K, Fin, kernel), make(name, K, Fin, kernel, graph=True)
    xd = dev(x)
    with torch.no_grad():
        want = plain(xd)
        y1 = captured(xd)
        first = y1.clone()
        y2 = captured(xd)
    torch.cuda.synchronize()
    assert y1.data_ptr() == y2.data_ptr() and captured._basis_image["count"] == 1
    assert torch.equal(first, want) and torch.equal(y2, want)


def test_network_equals_its_layers():
    torch.manual_seed(3)
    model = HealpyGCNN(4, np.arange(192), [HealpyBernstein(K=5, Fout=32), HealpyPool(1), HealpyBernstein(K=5, Fout=32)])
    x = dev(np.random.default_rng(4).standard_normal((2, 192, 1)))
    with torch.no_grad():
        y = model(x)
        parts = model[2](model[1](model[0](x)))
        pooled = model[0].forward_pool(x, "MAX")
    torch.cuda.synchronize()
    print("conv + pool in one pass:", pooled is not None)
    assert type(model[0]) is Bernstein and tuple(y.shape) == (2, 48, 32)
    assert rel_err(y.cpu().numpy(), parts.cpu().numpy()) < 2e-5
    if pooled is not None:
        assert rel_err(pooled.cpu().numpy(), model[1](model[0](x)).cpu().numpy()) < 2e-5


def test_conv_and_pool_in_one_pass_through_a_bernstein_layer():
    """The shape of the network above is too small for the pooled store; this one (six terms on the 8-neighbour stencil: the
    BFS-tile kernel, which pools in its store) is not -- same bits as the two layers."""
    name, K, Fin, Fout, N = "n16", 5, 16, 32, 2
    x, _, kernel = data(name, N, Fin, Fout, K)
    layer = make(name, K, Fin, kernel, activation="relu", use_bias=True)
    xd = dev(x)
    with torch.no_grad():
        pooled = layer.forward_pool(xd, "MAX")
        assert pooled is not None and tuple(pooled.shape) == (N, 768, Fout)
        two = HealpyPool(1)(layer(xd))
    torch.cuda.synchronize()
    assert torch.equal(pooled, two) and layer._basis_image["count"] == 1
