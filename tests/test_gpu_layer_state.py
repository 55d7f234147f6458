"""Layer state across calls: one long-lived layer driven through scripted sequences, in lockstep with the float64 model of
tests/layer_state_ref.py (pinned in tests/test_layer_state_host.py).

After every step that produces a map, a gradient or a statistic the runner asserts
  (a) the model, at the project's existing bounds: 2e-6 of max|ref| for fp32 / bf16x6 / f16x3, 1e-5 for bf16x3 with 16 or more
      contracted channels and 2e-5 below, five times that behind tanh, 2e-5 for gradients; outputs of a batch-normalised layer
      1e-5 and moving statistics 1e-6, the bounds of tests/test_gpu_batchnorm.py for the same quantities;
  (b) a fresh twin: a layer constructed at that moment from the long-lived layer's ``state_dict`` and constructor arguments
      (never ``graph=True``: a replay must give the plain launches' bits) and called once in the same mode on the same input --
      ``torch.equal``.  Same plan options, same batch, same route: same sums.  This is what catches a stale cache whose error is
      below any tolerance.  DSPH_OPT_STRIPS is pinned in every sequence (at its default the route may change with the batch).
No step of these sequences changes the summation order, so none is relaxed from (b): ``TALLY`` counts both kinds and every test
asserts that at most a fifth are relaxed.
"""

import copy
import functools
import warnings

import numpy as np
import pytest
import torch

import layer_state_ref as lsr
from bernstein_ref import csr as ell_csr
from deepsphere import _native, gnn_layers
from deepsphere.healpy_layers import HealpyChebyshev, HealpyPool
from deepsphere.healpy_networks import HealpyGCNN
from helpers import rel_err
from test_gpu_round3 import _csr, _grid_ell

pytestmark = pytest.mark.gpu

TOL_FP32_EQUIV = 2e-6   # fp32, bf16x6, f16x3 (test_gpu_round4 / round5 / bernstein)
TOL_BF16X3 = 1e-5       # 16 or more contracted channels; twice that below (test_gpu_round3 / round4)
TOL_GRAD = 2e-5         # (TOL_QWGRAD)
TOL_BN = 1e-5           # test_gpu_batchnorm.TOL: z of a batch-normalised map
TOL_MOVING = 1e-6       # test_gpu_batchnorm.TOL_MOVING

NEVER = {_native.OPT_STRIPS: _native.STRIPS_NEVER}
ALWAYS = {_native.OPT_STRIPS: _native.STRIPS_ALWAYS}
PREC_NAME = {_native.PREC_FP32: "fp32", _native.PREC_BF16X3: "bf16x3", _native.PREC_BF16X6: "bf16x6", _native.PREC_F16X3: "f16x3"}
BASIS = {gnn_layers.Chebyshev: "chebyshev", gnn_layers.Monomial: "monomial", gnn_layers.Bernstein: "bernstein"}

TALLY = {"compared": 0, "relaxed": 0}
WORST = {}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda()


def host(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def grid(nside):
    """-> (ELL columns, ELL values, the same fp32 L~ as a float64 CSR matrix) of the full sphere; one per module."""
    cols, vals = _grid_ell(nside)
    return cols, vals, _csr(cols, vals)


def conv_tol(layer):
    name = PREC_NAME[layer._prec_code()]
    tol = TOL_FP32_EQUIV if name != "bf16x3" else (TOL_BF16X3 if layer._Fin >= 16 else 2 * TOL_BF16X3)
    return tol * (5 if layer._act_code == _native.ACT_TANH else 1)


def out_tol(layer):
    return max(conv_tol(layer), TOL_BN) if layer.use_bn else conv_tol(layer)


def held(group, label, got, ref, tol):
    """(a): print, remember the worst of the group, assert."""
    got = host(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    assert np.isfinite(got).all(), f"{label}: non-finite values"
    err = rel_err(got, ref)
    WORST[group] = max(WORST.get(group, 0.0), err)
    print(f"  {label}: {group} {err:.2e} (bound {tol:.0e})")
    assert err <= tol, f"{label}: {group} {err:.3e} > {tol:.0e}"
    return err


def same_bits(label, got, twin, relaxed_because=None):
    """(b), counted; ``relaxed_because``: the step is held to (a) only."""
    TALLY["compared"] += 1
    if relaxed_because is not None:
        TALLY["relaxed"] += 1
        return
    assert torch.equal(got, twin), (f"{label}: not the bits of a fresh twin, max |diff| {float((got - twin).abs().max()):.3e} "
                                    f"of max |y| {float(twin.abs().max()):.3e}")


class Run:
    """One long-lived layer, its float64 model, and the steps of a sequence.  ``play`` applies a list of (step, args...)."""

    def __init__(self, cls, nside, K, Fin, Fout, seed=0, **kw):
        """``Fout=None``: the layer is constructed without one and takes its input's width."""
        cols, vals, Lt = grid(nside)
        self.M, self.Fin, self.Fout, self.kw, self.cls = cols.shape[0], Fin, Fin if Fout is None else Fout, kw, cls
        self._make = lambda **over: cls.from_prepared_ell(cols, vals, K, Fout=Fout, device="cuda:0", **{**kw, **over})
        self.rng = np.random.default_rng(1000 * Fin + 10 * self.Fout + K + seed)
        self.layer = self._make()
        self.layer.build((1, self.M, Fin))
        self.declared = set(vars(self.layer))  # a layer declares all it keeps at construction: play() holds it to that
        W, b = self.new_weights()
        with torch.no_grad():
            self.layer.kernel.copy_(dev(W))
            if b is not None:
                self.layer.bias.copy_(dev(b).reshape(1, 1, -1))
        self.model = lsr.LayerModel(Lt, K, W, b, use_bn=bool(kw.get("use_bn")), activation=kw.get("activation"), basis=BASIS[cls])
        self.inputs, self.start = {}, dict(TALLY)

    def new_weights(self):
        W = self.rng.standard_normal((self.layer._n_terms * self.Fin, self.Fout)) * self.layer._default_stddev(self.Fin, self.Fout)
        b = self.rng.standard_normal(self.Fout).astype(np.float32) if self.kw.get("use_bias") else None
        return W.astype(np.float32), b

    def x(self, N):
        """One input per batch size: (numpy, device tensor), drawn once, never written."""
        if N not in self.inputs:
            a = self.rng.standard_normal((N, self.M, self.Fin)).astype(np.float32)
            dy = (self.rng.standard_normal((N, self.M, self.Fout)) / np.sqrt(N * self.M)).astype(np.float32)
            self.inputs[N] = (a, dev(a), dy, dev(dy))
        return self.inputs[N]

    def twin(self):
        t = self._make(graph=False)
        t.build((1, self.M, self.Fin))
        t.load_state_dict(self.layer.state_dict())
        t.train(self.layer.training)
        t.x_absmax = self.layer.x_absmax
        return t

    def play(self, steps):
        for i, step in enumerate(steps):
            print(f"step {i}: {step}")
            getattr(self, step[0])(*step[1:])
        torch.cuda.synchronize()
        assert set(vars(self.layer)) == self.declared, f"attributes that appeared after build(): {sorted(set(vars(self.layer)) - self.declared)}"
        compared, relaxed = (TALLY[k] - self.start[k] for k in ("compared", "relaxed"))
        print(f"{compared} steps compared with a twin, {relaxed} relaxed")
        assert compared > 0 and 5 * relaxed <= compared

    # ---- what is checked after a step
    def moving(self, label, twin=None):
        bn = self.layer.bn
        held("moving mean", label, bn.running_mean, self.model.running_mean, TOL_MOVING)
        held("moving var", label, bn.running_var, self.model.running_var, TOL_MOVING)
        assert int(bn.num_batches_tracked) == self.model.num_batches_tracked
        if twin is not None:
            assert torch.equal(bn.running_mean, twin.bn.running_mean) and torch.equal(bn.running_var, twin.bn.running_var)

    # ---- steps
    def infer(self, N, keeps=None):
        """Inference without autograd; ``keeps``: whether the call must (True) / must not (False) have found its weight images."""
        a, xd, _, _ = self.x(N)
        twin = self.twin()
        before = getattr(self.layer, "_wkey", None)
        with torch.no_grad():
            y = self.layer(xd).clone()
            want = twin(xd)
        held("y", f"infer N={N}", y, self.model.infer(a), out_tol(self.layer))
        same_bits(f"infer N={N}", y, want)
        if keeps is not None and not self.layer._use_graph:
            assert (before == self.layer._wkey) == keeps, "kept weight images" if keeps else "weight images must have been re-packed"
        return y

    def train_nograd(self, N):
        """``training=True`` without autograd: the batch-norm kernels in place on the convolution's output."""
        a, xd, _, _ = self.x(N)
        twin = self.twin()
        with torch.no_grad():
            z = self.layer(xd, training=True).clone()
            want = twin(xd, training=True)
        held("z (batch statistics)", f"train, autograd off, N={N}", z, self.model.train_forward(a), out_tol(self.layer))
        same_bits(f"train, autograd off, N={N}", z, want)
        if self.layer.use_bn:
            self.moving(f"train, autograd off, N={N}", twin)

    def sgd(self, N, frozen=False, training=True):
        """A training forward and backward through autograd; then an SGD step on the layer and on the model (``frozen``: the
        parameters do not require grad, only the input does, and nothing is updated)."""
        a, xd, dy, dyd = self.x(N)
        twin, layer, label = self.twin(), self.layer, f"{'frozen ' if frozen else ''}training step N={N}"
        params = [p for p in (layer.kernel, layer.bias) if p is not None]
        for p in params:
            p.requires_grad_(not frozen)
            p.grad = None
        xg = xd.clone().requires_grad_(True)
        z = layer(xg, training=training)
        z.backward(dyd)
        want = twin(xd.clone().requires_grad_(True), training=training).detach()  # (the same mode: autograd on)
        ref = self.model.train_forward(a) if training else self.model.infer(a)
        held("z (batch statistics)" if (layer.use_bn and training) else "y", label, z, ref, out_tol(layer))
        same_bits(label, z.detach(), want)
        mask = host(z) if self.kw.get("activation") == "relu" else None
        dx = self.model.backward(a, dy, training=training, z_for_mask=mask)
        held("dx", label, xg.grad, dx, TOL_GRAD)
        if layer.use_bn and training:
            self.moving(label)
        if frozen:
            assert all(p.grad is None for p in params)
            for p in params:
                p.requires_grad_(True)
            return
        held("dkernel", label, layer.kernel.grad, self.model.grads["kernel"], TOL_GRAD)
        if layer.bias is not None:
            held("dbias", label, layer.bias.grad.reshape(-1), self.model.grads["bias"], TOL_GRAD)
        # a step that moves the largest weight by about a tenth of itself: far above every bound if the layer missed it
        lr = float(0.1 * np.abs(self.model.kernel).max() / np.abs(self.model.grads["kernel"]).max())
        with torch.no_grad():
            for p in params:
                p -= lr * p.grad
                p.grad = None
        self.model.sgd_step(lr)

    def frozen_train(self, N):
        self.sgd(N, frozen=True)

    def infer_autograd(self, N):
        """Inference with autograd on (the input requires grad): the convolution packs the raw kernel into the workspace."""
        self.sgd(N, frozen=True, training=False)

    def load_state(self):
        W, b = self.new_weights()
        sd = {k: v.clone() for k, v in self.layer.state_dict().items()}
        sd["kernel"] = dev(W)
        if b is not None:
            sd["bias"] = dev(b).reshape(1, 1, -1)
        self.layer.load_state_dict(sd)
        self.model.kernel, self.model.bias = W.astype(np.float64), None if b is None else b.astype(np.float64)

    def data_write(self):
        """A write through ``kernel.data`` moves no version counter: ``invalidate_weights`` is the documented way to say so."""
        version = self.layer.kernel._version
        self.layer.kernel.data.mul_(-0.75)
        assert self.layer.kernel._version == version
        self.layer.invalidate_weights()
        self.model.kernel = self.model.kernel * -0.75

    def bias_write(self):
        b = self.rng.standard_normal(self.Fout).astype(np.float32)
        with torch.no_grad():
            self.layer.bias.copy_(dev(b).reshape(1, 1, -1))
        self.model.bias = b.astype(np.float64)

    def stats_write(self):
        """New moving statistics, written in place as a checkpoint's would be."""
        m, v = self.rng.standard_normal(self.Fout).astype(np.float32), self.rng.uniform(0.5, 2.0, self.Fout).astype(np.float32)
        with torch.no_grad():
            self.layer.bn.running_mean.copy_(dev(m))
            self.layer.bn.running_var.copy_(dev(v))
        self.model.running_mean, self.model.running_var = m.astype(np.float64), v.astype(np.float64)

    def pool(self, N, pool_type):
        """``forward_pool`` against the model, the twin's ``forward_pool`` and ``HealpyPool`` of the twin's full output."""
        a, xd, _, _ = self.x(N)
        twin, full = self.twin(), self.twin()
        with torch.no_grad():
            y = self.layer.forward_pool(xd, pool_type)
            assert y is not None, "this shape pools in the convolution's store"
            want = twin.forward_pool(xd, pool_type)
            two = HealpyPool(1, pool_type)(full(xd))
        label = f"conv + pool {pool_type} N={N}"
        held("pooled y", label, y, self.model.pool(self.model.infer(a), pool_type), out_tol(self.layer))
        same_bits(label, y, want)
        if pool_type == "MAX":
            assert torch.equal(y, two), f"{label}: not the bits of the two layers"
        else:
            held("pooled y against the two layers", label, y, host(two).astype(np.float64), out_tol(self.layer))


STEADY = [("infer", 2), ("infer", 2, True), ("sgd", 2), ("infer", 2, False), ("infer", 2, True), ("load_state",), ("infer", 2, False),
          ("data_write",), ("infer", 2, False), ("frozen_train", 2), ("infer", 2), ("infer", 2, True)]


@pytest.mark.parametrize("cls", [gnn_layers.Chebyshev, gnn_layers.Monomial], ids=["chebyshev", "monomial"])
@pytest.mark.parametrize("Fin,Fout,K,act", [(4, 8, 5, "relu"), (16, 32, 5, "tanh"), (64, 64, 5, "relu"), (16, 32, 10, None), (5, 7, 5, "elu")],
                         ids=["4-8", "16-32", "64-64", "16-32-K10", "5-7"])
def test_steady_state_and_weight_updates(cls, Fin, Fout, K, act):
    """The kept weight images follow every way the weights can change: an optimiser step, ``load_state_dict``, a write through
    ``.data`` announced by ``invalidate_weights``, a training pass that leaves them alone.  (5 -> 7: x is copied into the
    workspace with padded channels; K = 10: per-pass image areas.)"""
    Run(cls, 32, K, Fin, Fout, use_bias=True, activation=act, plan_options=NEVER).play(STEADY)


@pytest.mark.parametrize("nside,Fin,Fout,options", [(32, 4, 8, NEVER), (32, 1, 16, NEVER), (128, 16, 32, ALWAYS)],
                         ids=["4-8", "1-16", "16-32-strips"])
def test_batch_changes(nside, Fin, Fout, options):
    """N = 1 -> 3 -> 2 -> 1 -> 4 on one layer: the class that packs four maps of a narrow layer into one item and ``N > 1`` in the
    key of the kept images, a workspace that grows and never shrinks; 16 -> 32 on the input-side strips.

    (Dropping ``(self.algo, N > 1)`` from the layer's key leaves this test green: the library keeps its own record of which
    images a workspace block holds, batch class included -- ``fused_images_key`` in csrc/cheb_fused.hip -- and re-packs by
    itself.  The term is a second line of defence; what this test holds is the outcome, through both.)"""
    run = Run(gnn_layers.Chebyshev, nside, 5, Fin, Fout, use_bias=True, activation="relu", plan_options=options)
    if options is ALWAYS:
        plan = run.layer._get_plan()
        for N in (1, 2, 3, 4):
            assert plan.strip_tiles(Fin, Fout, 5, run.layer._prec_code(), N=N) > 0, "the input-side strips take this shape"
    sizes = []
    for N in (1, 3, 2, 1, 4):
        run.play([("infer", N)])
        sizes.append(0 if run.layer._workspace is None else run.layer._workspace.numel())
    assert sizes == sorted(sizes), "the workspace grows with the batch and is kept when the batch shrinks"
    run.play([("infer", 4, True), ("infer", 1), ("infer", 1, True)])


TRAIN_EVAL = [("infer", 2), ("train_nograd", 2), ("infer", 2, False), ("sgd", 2), ("infer", 2, False), ("infer", 2, True),
              ("infer_autograd", 2), ("infer", 2), ("stats_write",), ("infer", 2, False), ("train_nograd", 3), ("infer", 3), ("infer", 2)]


@pytest.mark.parametrize("cls,K,Fin,Fout,act", [(gnn_layers.Chebyshev, 5, 4, 8, "elu"), (gnn_layers.Chebyshev, 5, 16, 32, "relu"),
                                                (gnn_layers.Bernstein, 3, 4, 8, "relu")], ids=["chebyshev-elu", "chebyshev-relu", "bernstein"])
def test_train_and_eval_with_batch_norm(cls, K, Fin, Fout, act):
    """``use_bn``: the fold of the moving statistics into weights and bias follows every training call -- the in-place kernels
    under ``no_grad`` move the statistics without moving a version counter -- and a pass with autograd on, which packs the raw
    kernel into the shared workspace, is not mistaken for the fold's images."""
    run = Run(cls, 16, K, Fin, Fout, use_bias=True, use_bn=True, activation=act, precision="fp32", plan_options=NEVER)
    run.play(TRAIN_EVAL)
    assert run.model.num_batches_tracked == 3


def test_more_than_nine_terms_without_Fout():
    """K = 10, 16 channels, ``Fout`` omitted, nside 16: the smallest shape at which a real plan is asked whether the layer runs as
    the chain of passes -- with the width ``build()`` resolved, forward and input gradient.  (``self.Fout`` = None went to
    ``dsph_plan_uses_chain``: ``TypeError`` in the first forward.)"""
    run = Run(gnn_layers.Chebyshev, 16, 10, 16, None, use_bias=True, activation="relu", plan_options=NEVER)
    assert run.layer.Fout is None and run.layer._Fout == 16 and tuple(run.layer.kernel.shape) == (160, 16)
    run.play([("infer", 2), ("sgd", 2)])


def test_bernstein_steady_state():
    """(16 -> 32 at the layer's default arithmetic, the three-term split on the transformed weights: measured 7.0e-6 - 9.5e-6 of
    max|y| over the sequence, held to 1e-5 like every three-term contraction over 16 or more channels here.)"""
    run = Run(gnn_layers.Bernstein, 16, 4, 16, 32, use_bias=True, activation="relu", plan_options=NEVER)
    run.play(STEADY)
    assert run.layer._basis_image["count"] >= 3


def test_data_write_on_a_layer_with_folded_batch_norm():
    """``invalidate_weights`` after a write through ``kernel.data`` must also reach the fold of the moving statistics, which is
    keyed on the same version counter."""
    run = Run(gnn_layers.Chebyshev, 16, 5, 4, 8, use_bias=True, use_bn=True, activation="relu", precision="fp32", plan_options=NEVER)
    run.play([("stats_write",), ("infer", 2), ("data_write",), ("infer", 2), ("infer", 2, True)])


@pytest.mark.parametrize("use_bn", [False, True], ids=["plain", "bn"])
@pytest.mark.parametrize("pool_type", ["MAX", "AVG"])
@pytest.mark.parametrize("Fin,Fout", [(1, 16), (16, 32)], ids=["1-16", "16-32"])
def test_forward_and_forward_pool_share_one_workspace(Fin, Fout, pool_type, use_bn):
    run = Run(gnn_layers.Chebyshev, 32, 5, Fin, Fout, use_bias=True, use_bn=use_bn, activation="relu", plan_options=NEVER)
    steps = [("stats_write",)] if use_bn else []
    run.play(steps + [("pool", 2, pool_type), ("infer", 2), ("pool", 2, pool_type), ("load_state",), ("pool", 2, pool_type), ("infer", 2),
                      ("pool", 2, pool_type)])


# ------------------------------------------------------------------------------------------------------ f16x3: the input scale

@functools.lru_cache(maxsize=None)
def f16_case():
    """x (N = 2, nside 128, 64 channels), W and the float64 convolution, once for the four cases; never written."""
    cols, vals, Lt = grid(128)
    rng = np.random.default_rng(128)
    x = rng.standard_normal((2, cols.shape[0], 64)).astype(np.float32)
    W = (rng.standard_normal((64 * 5, 64)) * 0.1).astype(np.float32)
    return x, W, lsr.LayerModel(Lt, 5, W).infer(x)


@pytest.mark.parametrize("graph", [False, True], ids=["plain", "graph"])
@pytest.mark.parametrize("absmax", ["reduced", "caller"])
def test_f16x3_scale_follows_the_input(absmax, graph):
    """One layer, one input buffer rewritten in place at scales 1, 2^6, 2^-9, 1.  The power of two x enters the f16 split with
    must follow it on every route to the quad strips, a captured graph included: finite, within 2e-6 of the model, the bits of a
    fresh twin; and, the factor being exact both ways, y / scale bit-equal across scales.  (Measured 7.7e-7 at every scale.  With
    the exponent missing from the capture key the replay at scale 2^6 split x 2^e beyond the f16 range: 18,677,760 of 25,165,824
    values of y non-finite.)"""
    cols, vals, _ = grid(128)
    x, W, ref = f16_case()
    layer = gnn_layers.Chebyshev.from_prepared_ell(cols, vals, 5, Fout=64, device="cuda:0", precision="f16x3", plan_options=ALWAYS, graph=graph)
    layer.build((1, cols.shape[0], 64))
    with torch.no_grad():
        layer.kernel.copy_(dev(W))
    assert layer._get_plan().strip_tiles(64, 64, 5, _native.PREC_F16X3, N=2) > 0, "the quad strips take this shape"
    x0 = dev(x)
    bound, buf, first = float(np.abs(x).max()), x0.clone(), None
    for scale in (1.0, 2.0 ** 6, 2.0 ** -9, 1.0):
        buf.copy_(x0 * scale)
        layer.x_absmax = bound * scale if absmax == "caller" else None
        twin = gnn_layers.Chebyshev.from_prepared_ell(cols, vals, 5, Fout=64, device="cuda:0", precision="f16x3", plan_options=ALWAYS,
                                                      x_absmax=layer.x_absmax)
        twin.build((1, cols.shape[0], 64))
        twin.load_state_dict(layer.state_dict())
        with torch.no_grad():
            y = layer(buf).clone()
            want = twin(buf)
        label = f"f16x3 scale {scale:g}"
        assert bool(torch.isfinite(y).all()), f"{label}: non-finite values ({int((~torch.isfinite(y)).sum())} of {y.numel()})"
        held("y", label, y, ref * scale, TOL_FP32_EQUIV)
        same_bits(label, y, want)
        first = y if first is None else first
        if not graph:
            assert torch.equal(y / scale, first), f"{label}: y / scale is not the bits of scale 1"


# ------------------------------------------------------------------------------------------------------ graph replay

def test_graph_replay_sees_a_bias_written_in_place():
    run = Run(gnn_layers.Chebyshev, 32, 5, 16, 32, use_bias=True, activation="relu", plan_options=NEVER, graph=True)
    y1 = run.infer(2)
    captured = run.layer._graph["graph"]
    run.play([("infer", 2), ("bias_write",), ("infer", 2)])
    assert run.layer._graph["graph"] is captured, "the bias is read through the same pointer: nothing to capture again"
    # the replay writes the one output buffer: what an earlier call returned now holds the latest values
    a, xd, _, _ = run.x(2)
    with torch.no_grad():
        r1 = run.layer(xd)
        kept = r1.clone()
        run.bias_write()
        r2 = run.layer(xd)
    assert r1.data_ptr() == r2.data_ptr() == run.layer._graph["out"].data_ptr()
    assert torch.equal(r1, r2) and not torch.equal(kept, r2) and not torch.equal(y1, kept)


@pytest.mark.parametrize("cls,K", [(gnn_layers.Chebyshev, 5), (gnn_layers.Bernstein, 4)], ids=["chebyshev", "bernstein"])
def test_graph_replay_follows_the_fold_and_the_basis_image(cls, K):
    """``graph=True`` on a layer whose kernels read derived weights: the fold of the moving statistics, Bernstein's basis image.
    Both are rewritten in place when their sources change; the captured forward must not replay over stale images."""
    run = Run(cls, 16, K, 16, 32, use_bias=True, use_bn=True, activation="relu", precision="fp32", plan_options=NEVER, graph=True)
    run.play([("infer", 2), ("infer", 2), ("stats_write",), ("infer", 2), ("train_nograd", 2), ("infer", 2), ("infer", 2),
              ("load_state",), ("infer", 2), ("sgd", 2), ("infer", 2), ("infer", 2)])
    if cls is gnn_layers.Bernstein:
        assert run.layer._basis_image["count"] >= 3


# ------------------------------------------------------------------------------------------------------ the residual block

@pytest.mark.parametrize("norm_type", ["batch_norm", "layer_norm"])
def test_residual_layer_between_inference_and_training(norm_type):
    """8 -> 8, K 3, nside 16: ``no_grad`` inference (native epilogue, ``bn_apply`` on the moving statistics) alternating with
    autograd training (``_BatchNormActFunction`` / the layer-norm kernels) on one block."""
    from deepsphere import healpix

    L = healpix.healpix_laplacian(16, mode="grid")
    M, F, K = L.shape[0], 8, 3
    kw = {"L": L, "K": K, "Fout": F, "precision": "fp32", "device": "cuda:0", "plan_options": NEVER}
    rng = np.random.default_rng(16)
    xs = [rng.standard_normal((N, M, F)).astype(np.float32) for N in (2, 3)]

    def make():
        res = gnn_layers.GCNN_ResidualLayer("CHEBY", dict(kw), activation="relu", use_bn=True, norm_type=norm_type, alpha=0.5)
        with torch.no_grad():
            res(dev(xs[0]))  # creates the weights and the two norm modules
        return res

    res = make()
    with torch.no_grad():
        for mod in (res.bn1, res.bn2):
            mod.weight.uniform_(0.5, 1.5)
            mod.bias.normal_()
    Lt = ell_csr(res.layer1._ell_cols, res.layer1._ell_vals)
    model = lsr.ResidualModel(lsr.LayerModel(Lt, K, host(res.layer1.kernel)), lsr.LayerModel(Lt, K, host(res.layer2.kernel)),
                              lsr.NormModel(norm_type, F, host(res.bn1.weight), host(res.bn1.bias)),
                              lsr.NormModel(norm_type, F, host(res.bn2.weight), host(res.bn2.bias)), activation="relu", alpha=0.5)
    start = dict(TALLY)
    for i, (training, which) in enumerate([(False, 0), (True, 0), (False, 0), (False, 1), (True, 1), (True, 0), (False, 0), (False, 0)]):
        x, label = xs[which], f"step {i}: residual {norm_type} training={training} N={xs[which].shape[0]}"
        twin = make()
        twin.load_state_dict(res.state_dict())
        for sub in (twin.layer1, twin.layer2):  # (the call that created the twin's modules left images of its first weights)
            sub.invalidate_weights()
        if training:
            xg = dev(x).requires_grad_(True)
            y = res(xg, training=True)
            y.backward(torch.ones_like(y) / y.numel())
            want = twin(dev(x).requires_grad_(True), training=True).detach()
            assert xg.grad is not None and res.layer1.kernel.grad is not None
        else:
            with torch.no_grad():
                y = res(dev(x), training=False)
                want = twin(dev(x), training=False)
        held("residual y", label, y, model.forward(x, training), TOL_BN)
        same_bits(label, y.detach(), want)
        if norm_type == "batch_norm":
            for mod, ours in ((res.bn1, model.norm1), (res.bn2, model.norm2)):
                held("moving mean", label, mod.running_mean, ours.running_mean, TOL_MOVING)
                held("moving var", label, mod.running_var, ours.running_var, TOL_MOVING)
                assert int(mod.num_batches_tracked) == ours.num_batches_tracked
    assert 5 * (TALLY["relaxed"] - start["relaxed"]) <= TALLY["compared"] - start["compared"]


# ------------------------------------------------------------------------------------------------------ the network's modes

NSIDE_NET = 16


@functools.lru_cache(maxsize=None)
def network_prototype():
    """Chebyshev (batch norm, bias, relu) -> pool -> Chebyshev -> pool at nside 16, weights created, never called: a fresh copy of
    it (``copy.deepcopy``: no plan, no workspace, no cache yet) is a fresh network."""
    torch.manual_seed(16)
    net = HealpyGCNN(NSIDE_NET, np.arange(12 * NSIDE_NET ** 2),
                     [HealpyChebyshev(K=5, Fout=16, use_bias=True, use_bn=True, activation="relu", device="cuda:0", plan_options=NEVER),
                      HealpyPool(1, "MAX"),
                      HealpyChebyshev(K=5, Fout=32, use_bias=True, activation="relu", device="cuda:0", plan_options=NEVER),
                      HealpyPool(1, "AVG")], graph_mode="grid")
    net[0].build((1, 12 * NSIDE_NET ** 2, 1))
    net[2].build((1, 12 * NSIDE_NET ** 2 // 4, 16))
    return net


def fresh_network(state=None, training=True, fused=True):
    net = copy.deepcopy(network_prototype())
    if state is not None:
        net.load_state_dict(state)
    net.train(training)
    if not fused:
        for layer in (net[0], net[2]):
            layer.forward_pool = lambda *a, **k: None
    return net


@pytest.mark.parametrize("grad", ["grad", "no_grad", "frozen"])
def test_network_mode_matrix(grad):
    """``training`` in {False, True, None} x ``model.train()`` / ``model.eval()`` on one long-lived network: outputs and every
    layer's moving statistics follow the rule ``Chebyshev.forward`` documents (``None`` follows ``self.training``), whether or
    not the convolution and the pooling behind it run in one pass -- also the bits and statistics of the same network, fresh,
    with that fusion disabled.  (``model.train()``, ``training=None``, autograd off or parameters frozen: the fused pass used to
    fold the moving statistics where the layer alone takes the batch's -- 0.65 / 0.68 of max|y| off, statistics not updated.)"""
    net = fresh_network()
    M = 12 * NSIDE_NET ** 2
    x = np.random.default_rng(3).standard_normal((2, M, 1)).astype(np.float32)
    xd = dev(x)
    with torch.no_grad():
        net[0].bn.running_mean.normal_()
        net[0].bn.running_var.uniform_(0.5, 2.0)
        assert net[0].forward_pool(xd, "MAX") is not None, "the first layer pools in its store when it may"
    if grad == "frozen":
        for p in net.parameters():
            p.requires_grad_(False)
    entries = []
    for layer in net:
        if isinstance(layer, gnn_layers.Chebyshev):
            m = lsr.LayerModel(ell_csr(layer._ell_cols, layer._ell_vals), layer.K, host(layer.kernel), host(layer.bias).reshape(-1),
                               use_bn=layer.use_bn, activation="relu")
            if layer.use_bn:
                m.running_mean, m.running_var = host(layer.bn.running_mean).astype(np.float64), host(layer.bn.running_var).astype(np.float64)
            entries.append(m)
        else:
            entries.append(("pool", layer.pool_type))
    model = lsr.NetworkModel(entries)
    start = dict(TALLY)
    for mode in (True, False):
        net.train(mode)
        for training in (False, True, None, True, None, False):
            label = f"network {grad} train()={mode} training={training}"
            batch_stats = mode if training is None else training
            unfused = fresh_network(net.state_dict(), training=mode, fused=False)
            if grad == "frozen":
                for p in unfused.parameters():
                    p.requires_grad_(False)
            with torch.set_grad_enabled(grad != "no_grad"), warnings.catch_warnings():
                warnings.simplefilter("ignore")
                y = net(xd, training=training).detach()
                want = unfused(xd, training=training).detach()
            ref = model.forward(x, [batch_stats, batch_stats])
            held("network y", label, y, ref, TOL_BN)
            for layer, ours in ((net[0], model.layers[0]),):
                held("moving mean", label, layer.bn.running_mean, ours.running_mean, TOL_MOVING)
                held("moving var", label, layer.bn.running_var, ours.running_var, TOL_MOVING)
                assert int(layer.bn.num_batches_tracked) == ours.num_batches_tracked, label
            same_bits(label, y, want)
            assert torch.equal(net[0].bn.running_mean, unfused[0].bn.running_mean), label
            assert torch.equal(net[0].bn.running_var, unfused[0].bn.running_var), label
    assert 5 * (TALLY["relaxed"] - start["relaxed"]) <= TALLY["compared"] - start["compared"]


def teardown_module(module):
    """The worst measured error per group and the share of steps relaxed from bit equality, for the record (``pytest -s``)."""
    print("\nworst per group:", {k: f"{v:.2e}" for k, v in sorted(WORST.items())})
    print(f"steps compared with a fresh twin: {TALLY['compared']}, relaxed from bit equality: {TALLY['relaxed']}")
