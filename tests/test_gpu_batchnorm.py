"""GPU tests of the batch-norm kernels (``dsph_bn_stats`` / ``dsph_bn_apply`` / ``dsph_bn_backward``, csrc/batch_norm.hip) and of
the layers on them (``pytest -m gpu``).

Yardstick: tests/batchnorm_ref.py (float64 numpy; held to torch's float64 autograd at 1e-12 by tests/test_batchnorm_host.py).
Error measure: ``helpers.rel_err`` (max-norm over max-norm).  Bounds: mean, var, z 1e-5 (the project's TOL); dy, dgamma, dshift
2e-5 (its gradient tolerance TOL_QWGRAD); the moving statistics 1e-6 against ``torch.nn.BatchNorm1d`` on the same device.

Data: seeded N(0, 1), one channel scaled by 3, all other channels offset by 10 -- a mean ten times the spread, where a variance
from E[y^2] - E[y]^2 in fp32 misses every bound by 10 x or more.  Every figure is printed before it is asserted.
"""

import copy
import functools

import numpy as np
import pytest
import torch

import batchnorm_ref as ref
from deepsphere import _native, healpix, utils
from deepsphere.gnn_layers import Bernstein, Chebyshev, GCNN_ResidualLayer, _BatchNormActFunction
from deepsphere.healpy_layers import HealpyChebyshev, HealpyPool
from deepsphere.healpy_networks import HealpyGCNN
from helpers import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5
TOL_GRAD = 2e-5
TOL_MOVING = 1e-6
EPS = 1e-5

# (rows, F): where the kernels can go wrong (there is no cap on F, so no shape at one)
SHAPES = [
    (15, 3),       # the reference's own layer test: 3 nodes x 5 maps
    (2, 4),        # the smallest legal batch
    (576, 1),      # a single channel
    (576, 2),      # the reference's Fout = 2
    (576, 5),      # the reference's Fout = 5
    (2304, 3),     # an odd, narrow channel count
    (1537, 16),    # rows that divide by nothing
    (6144, 64),    # the headline channel width
    (24576, 70),   # F % 4 != 0 across more than one 16-byte piece
    (36864, 5),    # many partials
]
ACT_CODES = {name: code for code, name in enumerate(ref.ACTS)}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda()


@functools.lru_cache(maxsize=None)
def data(rows, F):
    """y, dz, gamma, shift (float32 numpy); shared, never written."""
    rng = np.random.default_rng(1000 * F + rows)
    y = rng.standard_normal((rows, F))
    scaled = F // 2
    y[:, scaled] *= 3.0
    y[:, [c for c in range(F) if c != scaled]] += 10.0
    dz = rng.standard_normal((rows, F))
    gamma = rng.uniform(0.5, 1.5, F)
    shift = rng.standard_normal(F)
    return tuple(a.astype(np.float32) for a in (y, dz, gamma, shift))


@functools.lru_cache(maxsize=None)
def yardstick_forward(rows, F, act, affine):
    y, _, gamma, shift = data(rows, F)
    return ref.bn_forward(y, EPS, gamma if affine else None, shift if affine else None, act)


@pytest.mark.parametrize("affine", [True, False], ids=["gamma+shift", "plain"])
@pytest.mark.parametrize("act", ref.ACTS)
@pytest.mark.parametrize("rows,F", SHAPES)
def test_kernels_against_the_float64_yardstick(rows, F, act, affine):
    """Measured on an MI355X, largest over all cases: mean 4.8e-8, var 5.4e-8, z 7.9e-7; dy 2.6e-6, dgamma 9.4e-7, dshift 1.3e-6.

    (2, 4) is the hard one for dy: with two rows x^ = +-(1 - e), e = eps / 2 (var + eps) ~ 2e-5, and dy cancels to (g1 - g2) / 2 * (1 - x^2),
    4e-5 of |g|; one fp32 rounding of mean or rstd is 5 % of that (measured 6.8e-2 - 1.5e-1 with an fp32 backward).  The statistics and the
    backward therefore run in float64 and the backward takes the low parts of mean and rstd: 8.7e-9 - 2.6e-6 there."""
    y, dz, gamma, shift = data(rows, F)
    yd, dzd = dev(y), dev(dz)
    gd, sd = (dev(gamma), dev(shift)) if affine else (None, None)
    code = ACT_CODES[act]
    stats, _ = _native.bn_stats(yd, EPS)
    z = _native.bn_apply(yd, stats[0], stats[2], gd, sd, code)
    alias = yd.clone()
    assert _native.bn_apply(alias, stats[0], stats[2], gd, sd, code, out=alias) is alias
    dy, dgamma, dshift, _ = _native.bn_backward(yd, z if act != "none" else None, dzd, stats[0], stats[2], gd, code, mean_lo=stats[3], rstd_lo=stats[4])
    torch.cuda.synchronize()
    assert torch.equal(yd, dev(y)) and torch.equal(dzd, dev(dz)), "the inputs are read only"
    assert torch.equal(alias, z), "z over y: the same bits as into a fresh buffer"
    zh = z.cpu().numpy()
    mean, var, zref = yardstick_forward(rows, F, act, affine)
    dyref, dgref, dsref = ref.bn_backward(y, dz, EPS, gamma if affine else None, shift if affine else None, act, z_for_mask=zh)
    rstd = 1.0 / np.sqrt(var + EPS)
    errs = {"mean": rel_err(stats[0].cpu().numpy(), mean), "var": rel_err(stats[1].cpu().numpy(), var),
            "rstd": rel_err(stats[2].cpu().numpy(), rstd), "z": rel_err(zh, zref)}
    gerrs = {"dy": rel_err(dy.cpu().numpy(), dyref), "dgamma": rel_err(dgamma.cpu().numpy(), dgref),
             "dshift": rel_err(dshift.cpu().numpy(), dsref)}
    print(f"({rows}, {F}) {act} affine {int(affine)}:", {k: f"{v:.2e}" for k, v in {**errs, **gerrs}.items()})
    assert z.shape == yd.shape and dy.shape == yd.shape and dgamma.shape == (F,) and dshift.shape == (F,)
    assert all(e <= TOL for e in errs.values()), errs
    assert all(e <= TOL_GRAD for e in gerrs.values()), gerrs


@pytest.mark.parametrize("offset", [1, 2], ids=["4-byte aligned", "8-byte aligned"])
def test_maps_that_are_not_16_byte_aligned_take_narrower_accesses(offset):
    """F % 4 == 0 but the pointers do not allow 16 bytes per lane: the same numbers through 4- or 8-byte accesses."""
    rows, F = 1537, 16
    y, dz, gamma, shift = data(rows, F)

    def shifted(a):
        buf = torch.zeros(rows * F + offset, dtype=torch.float32, device="cuda")
        view = buf[offset:].view(rows, F)
        view.copy_(torch.as_tensor(a))
        assert view.data_ptr() % 16 == 4 * offset and view.is_contiguous()
        return view

    yd, dzd, gd, sd = shifted(y), shifted(dz), dev(gamma), dev(shift)
    stats, _ = _native.bn_stats(yd, EPS)
    z = _native.bn_apply(yd, stats[0], stats[2], gd, sd, _native.ACT_ELU, out=shifted(np.zeros_like(y)))
    dy, dgamma, dshift, _ = _native.bn_backward(yd, z, dzd, stats[0], stats[2], gd, _native.ACT_ELU, mean_lo=stats[3], rstd_lo=stats[4])
    torch.cuda.synchronize()
    mean, var, zref = yardstick_forward(rows, F, "elu", True)
    dyref, dgref, dsref = ref.bn_backward(y, dz, EPS, gamma, shift, "elu")
    errs = {"mean": rel_err(stats[0].cpu().numpy(), mean), "var": rel_err(stats[1].cpu().numpy(), var), "z": rel_err(z.cpu().numpy(), zref)}
    gerrs = {"dy": rel_err(dy.cpu().numpy(), dyref), "dgamma": rel_err(dgamma.cpu().numpy(), dgref),
             "dshift": rel_err(dshift.cpu().numpy(), dsref)}
    print(offset, {k: f"{v:.2e}" for k, v in {**errs, **gerrs}.items()})
    assert all(e <= TOL for e in errs.values()) and all(e <= TOL_GRAD for e in gerrs.values()), (errs, gerrs)


@pytest.mark.parametrize("rows,F", SHAPES)
def test_moving_statistics_as_torch_keeps_them(rows, F):
    y = data(rows, F)[0]
    N = 3 if rows % 3 == 0 else 1
    yd = dev(y).view(N, rows // N, F)
    rng = np.random.default_rng(F)
    rm0, rv0 = dev(rng.standard_normal(F)), dev(rng.uniform(0.5, 2.0, F))
    ours = torch.nn.BatchNorm1d(F, eps=1e-3, momentum=0.01, affine=True).cuda()
    theirs = copy.deepcopy(ours)
    for bn in (ours, theirs):
        bn.running_mean.copy_(rm0)
        bn.running_var.copy_(rv0)
    with torch.no_grad():
        z = _BatchNormActFunction.apply(yd, ours.weight, ours.bias, ours, _native.ACT_NONE, False)
        theirs.train()
        zt = theirs(yd.transpose(1, 2)).transpose(1, 2)
    torch.cuda.synchronize()
    em = rel_err(ours.running_mean.cpu().numpy(), theirs.running_mean.cpu().numpy())
    ev = rel_err(ours.running_var.cpu().numpy(), theirs.running_var.cpu().numpy())
    print(f"({rows}, {F}): running_mean {em:.2e} running_var {ev:.2e}, z against torch {rel_err(z.cpu().numpy(), zt.cpu().numpy()):.2e}")
    assert int(ours.num_batches_tracked) == 1 == int(theirs.num_batches_tracked)
    assert not torch.equal(ours.running_mean, rm0) and not torch.equal(ours.running_var, rv0)
    assert em <= TOL_MOVING and ev <= TOL_MOVING
    # and against the yardstick's update rule (unbiased variance)
    mean, var, _ = ref.bn_forward(y, 1e-3)
    rm, rv = ref.moving_update(rm0.cpu().numpy(), rv0.cpu().numpy(), mean, var, rows, 0.01)
    assert rel_err(ours.running_mean.cpu().numpy(), rm) <= TOL_MOVING and rel_err(ours.running_var.cpu().numpy(), rv) <= TOL_MOVING


def test_one_row_raises_what_torch_raises():
    bn = torch.nn.BatchNorm1d(4).cuda()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        _BatchNormActFunction.apply(torch.zeros(1, 1, 4, device="cuda"), None, None, bn, _native.ACT_NONE, False)
    assert int(bn.num_batches_tracked) == 0


@pytest.mark.parametrize("rows,F", SHAPES)
def test_two_calls_give_the_same_bits(rows, F):
    y, dz, gamma, shift = data(rows, F)
    yd, dzd, gd, sd = dev(y), dev(dz), dev(gamma), dev(shift)

    def run():
        stats, _ = _native.bn_stats(yd, EPS)
        z = _native.bn_apply(yd, stats[0], stats[2], gd, sd, _native.ACT_TANH)
        return (stats, z) + _native.bn_backward(yd, z, dzd, stats[0], stats[2], gd, _native.ACT_TANH, mean_lo=stats[3], rstd_lo=stats[4])[:3]

    first, second = run(), run()
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- the layers

@functools.lru_cache(maxsize=None)
def graph(name):
    L = healpix.healpix_laplacian(4) if name == "n4" else healpix.healpix_laplacian(8, indices=healpix.cap_indices(8))
    Lt, _ = utils.prepare_L(L, scale=0.75)
    return utils.csr_to_ell(Lt) + (L,)


def parent_epilogue(c, bn, bias, activation):
    """The composition the layers ran before the kernels: the host framework's batch norm on the transposed view, + bias, the
    activation, each its own op.  ``bn`` is updated like any training-mode call."""
    bn.train()
    y = bn(c.transpose(1, 2)).transpose(1, 2)
    if bias is not None:
        y = y + bias
    return y if activation is None else activation(y)


@pytest.mark.parametrize("name", ["n4", "n8cap"])
@pytest.mark.parametrize("cls,K,act,fn", [(Chebyshev, 5, "elu", torch.nn.functional.elu), (Bernstein, 3, "relu", torch.relu)],
                         ids=["chebyshev-elu", "bernstein-relu"])
def test_layer_against_the_composition_it_replaces(cls, K, act, fn, name):
    cols, vals, _ = graph(name)
    M, N, Fin, Fout = cols.shape[0], 2, 4, 5
    rng = np.random.default_rng(3)
    x, dy = dev(rng.standard_normal((N, M, Fin))), dev(rng.standard_normal((N, M, Fout)))
    torch.manual_seed(1)
    layer = cls.from_prepared_ell(cols, vals, K, Fout=Fout, use_bn=True, use_bias=True, activation=act, precision="fp32", device="cuda:0")
    twin = cls.from_prepared_ell(cols, vals, K, Fout=Fout, precision="fp32", device="cuda:0")  # no epilogue: the convolution alone
    layer.build((N, M, Fin))
    twin.build((N, M, Fin))
    with torch.no_grad():
        twin.kernel.copy_(layer.kernel)
    bias_p = layer.bias.detach().clone().requires_grad_(True)
    bn_p = copy.deepcopy(layer.bn)

    xp = x.clone().requires_grad_(True)
    want = parent_epilogue(twin(xp), bn_p, bias_p, fn)
    want.backward(dy)
    xn = x.clone().requires_grad_(True)
    got = layer(xn, training=True)
    got.backward(dy)
    with torch.no_grad():  # the autograd-off branch of the same layer: in place on the convolution's output
        got_ng = layer(x, training=True)
    torch.cuda.synchronize()
    ey = rel_err(got.detach().cpu().numpy(), want.detach().cpu().numpy())
    eng = rel_err(got_ng.cpu().numpy(), want.detach().cpu().numpy())
    eg = {"x": rel_err(xn.grad.cpu().numpy(), xp.grad.cpu().numpy()),
          "kernel": rel_err(layer.kernel.grad.cpu().numpy(), twin.kernel.grad.cpu().numpy()),
          "bias": rel_err(layer.bias.grad.cpu().numpy(), bias_p.grad.cpu().numpy())}
    print(f"{cls.__name__} {name}: y {ey:.2e} (autograd off {eng:.2e}),", {k: f"{v:.2e}" for k, v in eg.items()})
    assert tuple(layer.bias.grad.shape) == (1, 1, Fout) and int(layer.bn.num_batches_tracked) == 2
    assert ey <= TOL and eng <= TOL
    assert all(e <= TOL_GRAD for e in eg.values()), eg
    assert set(layer.state_dict()) == {"kernel", "bias", "bn.running_mean", "bn.running_var", "bn.num_batches_tracked"}


def test_callable_activation_without_a_code_runs_after_the_kernel():
    cols, vals, _ = graph("n4")
    N, M, Fin, Fout = 2, cols.shape[0], 4, 5
    x = dev(np.random.default_rng(5).standard_normal((N, M, Fin)))
    torch.manual_seed(2)
    layer = Chebyshev.from_prepared_ell(cols, vals, 3, Fout=Fout, use_bn=True, use_bias=True, activation="softplus", precision="fp32",
                                        device="cuda:0")
    twin = Chebyshev.from_prepared_ell(cols, vals, 3, Fout=Fout, precision="fp32", device="cuda:0")
    layer.build((N, M, Fin))
    twin.build((N, M, Fin))
    with torch.no_grad():
        twin.kernel.copy_(layer.kernel)
        want = parent_epilogue(twin(x), copy.deepcopy(layer.bn), layer.bias, torch.nn.functional.softplus)
        got = layer(x, training=True)
    torch.cuda.synchronize()
    assert rel_err(got.cpu().numpy(), want.cpu().numpy()) <= TOL


def _residual_pair(alpha=0.5):
    """Two residual layers with the same weights and batch-norm state (built apart: a layer owns its plan) and an input."""
    cols, vals, L = graph("n4")
    x = dev(np.random.default_rng(6).standard_normal((3, cols.shape[0], 8)))

    def make():
        kw = {"L": L, "K": 3, "Fout": 8, "precision": "fp32", "device": "cuda:0"}
        res = GCNN_ResidualLayer("CHEBY", kw, activation="relu", use_bn=True, norm_type="batch_norm", alpha=alpha)
        with torch.no_grad():
            res(x)  # creates the weights and bn1 / bn2
        return res

    torch.manual_seed(4)
    res, twin = make(), make()
    with torch.no_grad():
        for bn in (res.bn1, res.bn2):
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_()
            bn.running_mean.normal_()
            bn.running_var.uniform_(0.5, 2.0)
    twin.load_state_dict(res.state_dict())
    return res, twin, x


def parent_residual(res, x, training):
    """GCNN_ResidualLayer.forward with the host framework's batch norm on the transposed view, as before the kernels."""
    def norm(mod, h):
        mod.train(training)
        return mod(h.transpose(1, 2)).transpose(1, 2)

    h = norm(res.bn1, res.layer1(x, training=training))
    h = norm(res.bn2, res.layer2(h, training=training))
    return torch.relu(h + res.alpha * x)


def test_residual_layer_training_against_the_composition_it_replaces():
    res, twin, x = _residual_pair()
    dy = dev(np.random.default_rng(8).standard_normal(tuple(x.shape)))
    xp = x.clone().requires_grad_(True)
    want = parent_residual(twin, xp, True)
    want.backward(dy)
    xn = x.clone().requires_grad_(True)
    got = res(xn, training=True)
    got.backward(dy)
    torch.cuda.synchronize()
    ey = rel_err(got.detach().cpu().numpy(), want.detach().cpu().numpy())
    names = ["layer1.kernel", "layer2.kernel", "bn1.weight", "bn1.bias", "bn2.weight", "bn2.bias"]
    ours, theirs = dict(res.named_parameters()), dict(twin.named_parameters())
    eg = {n: rel_err(ours[n].grad.cpu().numpy(), theirs[n].grad.cpu().numpy()) for n in names}
    eg["x"] = rel_err(xn.grad.cpu().numpy(), xp.grad.cpu().numpy())
    em = {n: rel_err(getattr(getattr(res, b), s).cpu().numpy(), getattr(getattr(twin, b), s).cpu().numpy())
          for b in ("bn1", "bn2") for s in ("running_mean", "running_var") for n in [f"{b}.{s}"]}
    print(f"residual, training: y {ey:.2e}", {k: f"{v:.2e}" for k, v in {**eg, **em}.items()})
    assert ey <= TOL and all(e <= TOL_GRAD for e in eg.values()), (ey, eg)
    assert all(e <= TOL_MOVING for e in em.values()), em
    assert int(res.bn1.num_batches_tracked) == int(twin.bn1.num_batches_tracked) == 1


def test_residual_layer_inference_on_the_moving_statistics():
    res, twin, x = _residual_pair()
    before = res.bn1.running_mean.clone()
    with torch.no_grad():
        want = parent_residual(twin, x, False)
        got = res(x, training=False)
    with_grad = res(x.clone().requires_grad_(True), training=False)  # autograd on: the host framework's ops, unchanged
    torch.cuda.synchronize()
    e, eg = rel_err(got.cpu().numpy(), want.cpu().numpy()), rel_err(with_grad.detach().cpu().numpy(), want.cpu().numpy())
    print(f"residual, inference: y {e:.2e}, with autograd {eg:.2e}")
    assert e <= TOL and eg <= TOL and with_grad.requires_grad
    assert torch.equal(before, res.bn1.running_mean) and int(res.bn1.num_batches_tracked) == 0


def test_quick_start_training_step_never_enters_the_host_batch_norm(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("torch.nn.functional.batch_norm was called")

    monkeypatch.setattr(torch.nn.functional, "batch_norm", refuse)
    torch.manual_seed(0)
    nside = 16
    conv = lambda Fout: HealpyChebyshev(K=10, Fout=Fout, use_bias=True, use_bn=True, activation="relu")  # noqa: E731
    model = HealpyGCNN(nside, np.arange(12 * nside * nside),
                       [conv(5), HealpyPool(p=1), conv(5), HealpyPool(p=1), conv(5), HealpyPool(p=1), conv(2)])
    x = dev(np.random.default_rng(2).standard_normal((3, 12 * nside * nside, 1)))
    with torch.no_grad():
        before = model(x).clone()
    convs = [layer for layer in model if isinstance(layer, Chebyshev)]
    assert len(convs) == 4 and all(float(c.bn.running_mean.abs().max()) == 0.0 for c in convs)
    out = model(x, training=True)
    out.square().mean().backward()
    with torch.no_grad():
        after = model(x)
    torch.cuda.synchronize()
    for n, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, n
    assert all(float(c.bn.running_mean.abs().max()) > 0.0 and int(c.bn.num_batches_tracked) == 1 for c in convs)
    assert tuple(after.shape) == tuple(before.shape) == (3, 12 * (nside // 8) ** 2, 2)
    assert not torch.equal(after, before), "the folded inference forward sees the moved statistics"


def test_training_forward_under_graph_capture():
    cols, vals, _ = graph("n4")
    N, M, Fin, Fout = 2, cols.shape[0], 4, 8
    x = dev(np.random.default_rng(9).standard_normal((N, M, Fin)))
    torch.manual_seed(5)
    layer = Chebyshev.from_prepared_ell(cols, vals, 5, Fout=Fout, use_bn=True, use_bias=True, activation="relu", precision="fp32",
                                        device="cuda:0")
    with torch.no_grad():
        eager = layer(x, training=True).clone()  # the warm-up: tables, workspace, weight images
        out = torch.zeros_like(eager)
        g = torch.cuda.CUDAGraph()
        cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                out.copy_(layer(x, training=True))
        cur.wait_stream(side)
        tracked = int(layer.bn.num_batches_tracked)
        g.replay()
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    assert int(layer.bn.num_batches_tracked) == tracked + 2, "the counter and the moving statistics move inside the graph"
