"""The float64 model of a layer's state (tests/layer_state_ref.py) pinned before anything is measured against it: the same
train / eval / train sequence through ``torch.nn.BatchNorm1d`` and plain ``torch`` ops in float64 on the CPU, autograd for the
gradients.  Outputs, gradients, updated parameters and moving statistics must agree to 1e-12 (``helpers.rel_err``).  No GPU."""

import numpy as np
import pytest
import torch

import layer_state_ref as lsr
from helpers import load_case, rel_err

TOL = 1e-12
ACT = {None: lambda v: v, "relu": torch.relu, "elu": torch.nn.functional.elu, "tanh": torch.tanh}


def torch_conv(Ld, x, kernel, K, basis):
    """sum_k T_k(L~) x W_k with dense float64 torch ops, the planes stacked as the layer documents (row f*K + k)."""
    planes = [x]
    for k in range(1, K):
        nxt = torch.einsum("mp,npf->nmf", Ld, planes[-1])
        planes.append(nxt if basis == "monomial" or k == 1 else 2.0 * nxt - planes[-2])
    xs = torch.stack(planes, dim=-1)  # (N, M, Fin, K)
    N, M, Fin, _ = xs.shape
    return (xs.reshape(N * M, Fin * K) @ kernel).reshape(N, M, -1)


class TorchLayer:
    def __init__(self, Lt, K, kernel, bias, use_bn, activation, basis):
        self.Ld = torch.as_tensor(Lt.toarray(), dtype=torch.float64)
        self.K, self.basis, self.act = K, basis, ACT[activation]
        self.kernel = torch.tensor(kernel, dtype=torch.float64, requires_grad=True)
        self.bias = None if bias is None else torch.tensor(bias, dtype=torch.float64, requires_grad=True)
        self.bn = torch.nn.BatchNorm1d(kernel.shape[1], eps=1e-5, momentum=0.1, affine=False).double() if use_bn else None

    def __call__(self, x, training):
        y = torch_conv(self.Ld, x, self.kernel, self.K, self.basis)
        if self.bn is not None:
            self.bn.train(training)
            y = self.bn(y.transpose(1, 2)).transpose(1, 2)
        if self.bias is not None:
            y = y + self.bias
        return self.act(y)

    def sgd(self, lr):
        with torch.no_grad():
            for p in (self.kernel, self.bias):
                if p is not None and p.grad is not None:
                    p -= lr * p.grad
                    p.grad = None


@pytest.mark.parametrize("basis,use_bn,activation,use_bias", [
    ("chebyshev", True, "elu", True), ("chebyshev", True, "relu", True), ("monomial", True, "tanh", False),
    ("chebyshev", False, "relu", True), ("monomial", False, None, True), ("chebyshev", True, None, False)])
def test_train_eval_train_sequence_against_torch(basis, use_bn, activation, use_bias):
    case = load_case("n4_k5")
    Lt, K, Fin, Fout, N = case["Lt"].astype(np.float64), 4, 3, 5, 2
    M = Lt.shape[0]
    rng = np.random.default_rng(5)
    kernel = rng.standard_normal((Fin * K, Fout)) * 0.3
    bias = rng.standard_normal(Fout) if use_bias else None
    model = lsr.LayerModel(Lt, K, kernel, bias, use_bn=use_bn, activation=activation, basis=basis)
    theirs = TorchLayer(Lt, K, kernel, bias, use_bn, activation, basis)
    errs = {}

    def stats(tag):
        if use_bn:
            errs[tag + " mean"] = rel_err(model.running_mean, theirs.bn.running_mean.numpy())
            errs[tag + " var"] = rel_err(model.running_var, theirs.bn.running_var.numpy())
            assert model.num_batches_tracked == int(theirs.bn.num_batches_tracked)

    for step, training in enumerate([False, True, False, True, True, False]):
        x = rng.standard_normal((N + step % 2, M, Fin))
        dy = rng.standard_normal((N + step % 2, M, Fout))
        xt = torch.tensor(x, requires_grad=True)
        want = theirs(xt, training)
        got = model.train_forward(x) if training else model.infer(x)
        errs[f"{step} y"] = rel_err(got, want.detach().numpy())
        stats(str(step))
        want.backward(torch.as_tensor(dy))
        dx = model.backward(x, dy, training=training)
        errs[f"{step} dx"] = rel_err(dx, xt.grad.numpy())
        errs[f"{step} dkernel"] = rel_err(model.grads["kernel"], theirs.kernel.grad.numpy())
        if use_bias:
            errs[f"{step} dbias"] = rel_err(model.grads["bias"], theirs.bias.grad.numpy())
        if training:
            model.sgd_step(0.05)
            theirs.sgd(0.05)
            errs[f"{step} kernel"] = rel_err(model.kernel, theirs.kernel.detach().numpy())
        else:
            theirs.kernel.grad = None
            if use_bias:
                theirs.bias.grad = None
    print({k: f"{v:.1e}" for k, v in errs.items()})
    assert all(e <= TOL for e in errs.values()), errs
    assert model.num_batches_tracked == (3 if use_bn else 0)


def test_bernstein_sequence_keeps_the_same_books():
    """The Bernstein convolution is ``bernstein_ref``'s (pinned in test_bernstein_host.py); here the epilogue and the books
    around it, against the same torch modules fed that convolution."""
    case = load_case("n4_k5")
    Lt, K, Fin, Fout, N = case["Lt"].astype(np.float64), 3, 2, 4, 2
    rng = np.random.default_rng(6)
    kernel, bias = rng.standard_normal((Fin * (K + 1), Fout)), rng.standard_normal(Fout)
    model = lsr.LayerModel(Lt, K, kernel, bias, use_bn=True, activation="relu", basis="bernstein")
    bn = torch.nn.BatchNorm1d(Fout, eps=1e-5, momentum=0.1, affine=False).double()
    for training in (True, False, True):
        x = rng.standard_normal((N, Lt.shape[0], Fin))
        c = torch.as_tensor(model.conv(x))
        bn.train(training)
        want = torch.relu(bn(c.transpose(1, 2)).transpose(1, 2) + torch.as_tensor(bias))
        got = model.train_forward(x) if training else model.infer(x)
        assert rel_err(got, want.numpy()) <= TOL
        assert rel_err(model.running_mean, bn.running_mean.numpy()) <= TOL and rel_err(model.running_var, bn.running_var.numpy()) <= TOL


@pytest.mark.parametrize("kind", ["batch_norm", "layer_norm"])
def test_residual_model_against_torch(kind):
    case = load_case("n4_k5")
    Lt, K, F, N = case["Lt"].astype(np.float64), 3, 4, 2
    M = Lt.shape[0]
    rng = np.random.default_rng(7)
    ks = [rng.standard_normal((F * K, F)) * 0.3 for _ in range(2)]
    gb = [(rng.uniform(0.5, 1.5, F), rng.standard_normal(F)) for _ in range(2)]
    model = lsr.ResidualModel(lsr.LayerModel(Lt, K, ks[0]), lsr.LayerModel(Lt, K, ks[1]),
                              lsr.NormModel(kind, F, *gb[0]), lsr.NormModel(kind, F, *gb[1]), activation="relu", alpha=0.5)
    layers = [TorchLayer(Lt, K, k, None, False, None, "chebyshev") for k in ks]
    norms = []
    for g, b in gb:
        mod = (torch.nn.BatchNorm1d(F, eps=1e-3, momentum=0.01) if kind == "batch_norm" else torch.nn.LayerNorm(F, eps=1e-3)).double()
        with torch.no_grad():
            mod.weight.copy_(torch.as_tensor(g))
            mod.bias.copy_(torch.as_tensor(b))
        norms.append(mod)
    for training in (False, True, False, True):
        x = rng.standard_normal((N, M, F))
        with torch.no_grad():
            v = torch.as_tensor(x)
            for layer, mod in zip(layers, norms):
                mod.train(training)
                v = layer(v, training)
                v = mod(v.transpose(1, 2)).transpose(1, 2) if kind == "batch_norm" else mod(v)
            want = torch.relu(v + 0.5 * torch.as_tensor(x))
        assert rel_err(model.forward(x, training), want.numpy()) <= TOL
        if kind == "batch_norm":
            for ours, mod in zip((model.norm1, model.norm2), norms):
                assert rel_err(ours.running_mean, mod.running_mean.numpy()) <= TOL
                assert rel_err(ours.running_var, mod.running_var.numpy()) <= TOL
                assert ours.num_batches_tracked == int(mod.num_batches_tracked)


def test_network_model_and_pool_against_torch():
    case = load_case("n4_k5")
    Lt, K, N = case["Lt"].astype(np.float64), 3, 2
    M = Lt.shape[0]
    rng = np.random.default_rng(8)
    k1, b1 = rng.standard_normal((2 * K, 4)), rng.standard_normal(4)
    first = lsr.LayerModel(Lt, K, k1, b1, use_bn=True, activation="relu")
    net = lsr.NetworkModel([first, ("pool", "MAX"), ("pool", "AVG")])
    theirs = TorchLayer(Lt, K, k1, b1, True, "relu", "chebyshev")
    for training in (True, False):
        x = rng.standard_normal((N, M, 2))
        with torch.no_grad():
            v = theirs(torch.as_tensor(x), training).transpose(1, 2)
            want = torch.nn.functional.avg_pool1d(torch.nn.functional.max_pool1d(v, 4), 4).transpose(1, 2)
        got = net.forward(x, [training])
        assert got.shape == (N, M // 16, 4) and rel_err(got, want.numpy()) <= TOL
    assert first.num_batches_tracked == 1
