"""A float64 model of what a graph-convolution layer holds from one call to the next, plain numpy (not collected by pytest).

``LayerModel`` keeps the state of one ``gnn_layers.Chebyshev`` / ``Monomial`` / ``Bernstein``: kernel, bias, the batch norm's moving
mean and variance with ``num_batches_tracked``, eps, momentum, activation and basis.  It answers the operations the layer answers --
``infer``, ``train_forward``, ``backward``, ``sgd_step``, ``pool`` -- by composing the yardsticks the per-call tests already use
(``oracle/cheb_oracle.py``, ``batchnorm_ref.py``, ``bernstein_ref.py``, ``layernorm_ref.py``); nothing is restated here but the order
BN -> bias -> activation and the bookkeeping between calls.  ``ResidualModel`` and ``NetworkModel`` stack it as
``GCNN_ResidualLayer`` and ``HealpyGCNN`` stack the layers.  Nothing of ``deepsphere`` is imported.
"""

import numpy as np
from scipy import sparse

import batchnorm_ref as bnref
import bernstein_ref as bref
import layernorm_ref as lnref
from oracle import cheb_oracle as orc

_BN_ACT = {None: "none", "linear": "none", "relu": "relu", "elu": "elu", "sigmoid": "sigmoid", "tanh": "tanh"}


def _f64(a):
    return None if a is None else np.array(a, dtype=np.float64)


class LayerModel:
    """y = act(BN(conv(x)) + bias); ``basis``: "chebyshev" | "monomial" (K terms) | "bernstein" (order K: K + 1 terms)."""

    def __init__(self, Lt, K, kernel, bias=None, use_bn=False, activation=None, basis="chebyshev", eps=1e-5, momentum=0.1):
        self.Lt = sparse.csr_matrix(Lt, dtype=np.float64)
        self.K, self.basis, self.activation = int(K), basis, activation
        self.kernel = _f64(kernel)
        Fout = self.kernel.shape[1]
        self.bias = None if bias is None else _f64(bias).reshape(Fout)
        self.use_bn, self.eps, self.momentum = bool(use_bn), float(eps), float(momentum)
        self.running_mean, self.running_var, self.num_batches_tracked = np.zeros(Fout), np.ones(Fout), 0
        self.grads = {}

    # ---- the linear part and its adjoints: the per-call yardsticks
    def conv(self, x):
        if self.basis == "chebyshev":
            return orc.chebyshev_forward(self.Lt, x, self.kernel, self.K)
        if self.basis == "monomial":
            return orc.monomial_forward(self.Lt, x, self.kernel, self.K)
        return bref.forward(self.Lt, x, self.kernel, self.K)

    def conv_backward(self, x, dc):
        """-> (dx, dkernel) of <conv(x), dc>."""
        if self.basis == "chebyshev":
            return orc.chebyshev_backward(self.Lt, x, self.kernel, self.K, dc)
        if self.basis == "bernstein":
            return bref.grad_x(self.Lt, self.kernel, self.K, dc), bref.grad_w(self.Lt, np.asarray(x, dtype=np.float64), self.K, dc)
        x = np.asarray(x, dtype=np.float64)
        Fin, Fout = x.shape[-1], self.kernel.shape[1]
        dW = np.einsum("knmf,nmo->fko", orc.monomial_planes(self.Lt, x, self.K), dc).reshape(Fin * self.K, Fout)
        Wr, LtT = self.kernel.reshape(Fin, self.K, Fout), self.Lt.T.tocsr()
        dx = sum(orc.monomial_planes(LtT, dc @ Wr[:, k, :].T, k + 1)[k] for k in range(self.K))
        return dx, dW

    def _act(self, v):
        return v if _BN_ACT[self.activation] == "none" else orc.ACTIVATIONS[self.activation](v)

    # ---- the operations of the layer
    def infer(self, x):
        """The moving statistics (if any), left untouched."""
        c = self.conv(x)
        if self.use_bn:
            c = (c - self.running_mean) / np.sqrt(self.running_var + self.eps)
        return self._act(c if self.bias is None else c + self.bias)

    def train_forward(self, x):
        """Batch statistics, and the moving-statistics update ``torch.nn.BatchNorm1d`` makes (unbiased variance).  Without batch
        norm the mode changes nothing."""
        if not self.use_bn:
            return self.infer(x)
        c = self.conv(x)
        mean, var, z = bnref.bn_forward(c, self.eps, shift=self.bias, act=_BN_ACT[self.activation])
        rows = c.shape[0] * c.shape[1]
        self.running_mean, self.running_var = bnref.moving_update(self.running_mean, self.running_var, mean, var, rows, self.momentum)
        self.num_batches_tracked += 1
        return z

    def backward(self, x, dy, training=True, z_for_mask=None):
        """Gradients of <forward(x), dy> in the mode ``training`` -> dx; dkernel and dbias are kept in ``self.grads`` for
        ``sgd_step``.  ``z_for_mask``: as ``batchnorm_ref.bn_backward`` (the ReLU mask of the output under test)."""
        dy = np.asarray(dy, dtype=np.float64)
        act = _BN_ACT[self.activation]
        c = self.conv(x)
        if self.use_bn and training:
            dc, _, dshift = bnref.bn_backward(c, dy, self.eps, shift=self.bias, act=act, z_for_mask=z_for_mask)
        else:
            s = 1.0 / np.sqrt(self.running_var + self.eps) if self.use_bn else 1.0
            pre = (c - self.running_mean) * s if self.use_bn else c
            z = self._act(pre if self.bias is None else pre + self.bias)
            if act == "relu" and z_for_mask is not None:
                z = np.asarray(z_for_mask, dtype=np.float64)
            g = dy * bnref._act_grad_from_output(z, act)
            dshift = g.reshape(-1, g.shape[-1]).sum(axis=0)
            dc = g * s
        dx, dW = self.conv_backward(x, dc)
        self.grads = {"kernel": dW, "bias": None if self.bias is None else dshift}
        return dx

    def sgd_step(self, lr):
        self.kernel = self.kernel - lr * self.grads["kernel"]
        if self.bias is not None and self.grads.get("bias") is not None:
            self.bias = self.bias - lr * self.grads["bias"]
        self.grads = {}

    @staticmethod
    def pool(y, pool_type="MAX"):
        return orc.healpy_pool(y, 1, pool_type)


class NormModel:
    """The norm module of a residual block: Keras-style batch norm (eps 1e-3, torch momentum 0.01, gamma and beta) with its moving
    statistics, or layer norm over the channels (eps 1e-3)."""

    def __init__(self, kind, F, gamma=None, beta=None, eps=1e-3, momentum=0.01):
        self.kind, self.eps, self.momentum = kind, eps, momentum
        self.gamma = np.ones(F) if gamma is None else _f64(gamma)
        self.beta = np.zeros(F) if beta is None else _f64(beta)
        self.running_mean, self.running_var, self.num_batches_tracked = np.zeros(F), np.ones(F), 0

    def __call__(self, v, training):
        if self.kind == "layer_norm":
            return lnref.ln_forward(v, self.eps, gamma=self.gamma, beta=self.beta)[0]
        if not training:
            return orc.keras_batch_norm(np.asarray(v, dtype=np.float64), training=False, moving_mean=self.running_mean,
                                        moving_var=self.running_var, gamma=self.gamma, beta=self.beta, eps=self.eps)
        mean, var, z = bnref.bn_forward(v, self.eps, gamma=self.gamma, shift=self.beta)
        rows = int(np.prod(np.shape(v)[:-1]))
        self.running_mean, self.running_var = bnref.moving_update(self.running_mean, self.running_var, mean, var, rows, self.momentum)
        self.num_batches_tracked += 1
        return z


class ResidualModel:
    """in -> layer1 -> norm1 -> layer2 -> norm2 -> act(out + alpha * in), as ``GCNN_ResidualLayer`` with ``use_bn``."""

    def __init__(self, layer1, layer2, norm1, norm2, activation="relu", alpha=1.0):
        self.layer1, self.layer2, self.norm1, self.norm2, self.activation, self.alpha = layer1, layer2, norm1, norm2, activation, alpha

    def forward(self, x, training):
        x = np.asarray(x, dtype=np.float64)
        step = (lambda m, v: m.train_forward(v)) if training else (lambda m, v: m.infer(v))
        v = self.norm1(step(self.layer1, x), training)
        v = self.norm2(step(self.layer2, v), training)
        return orc.ACTIVATIONS[self.activation](v + self.alpha * x)


class NetworkModel:
    """A ``HealpyGCNN`` of ``LayerModel`` and ("pool", type) entries.  ``forward(x, modes)``: ``modes[i]`` says whether graph
    layer i runs on batch statistics -- the caller resolves ``training=None`` against each layer's own mode, the rule
    ``Chebyshev.forward`` documents."""

    def __init__(self, entries):
        self.entries = list(entries)

    @property
    def layers(self):
        return [e for e in self.entries if isinstance(e, LayerModel)]

    def forward(self, x, modes):
        modes = list(modes)
        for e in self.entries:
            if isinstance(e, LayerModel):
                x = e.train_forward(x) if modes.pop(0) else e.infer(x)
            else:
                x = LayerModel.pool(x, e[1])
        return x
