"""CPU tests of the batch-norm path: the float64 yardstick (tests/batchnorm_ref.py) against torch's float64 autograd, the four
entry points of the C ABI (exported, bound, arguments validated before any HIP call), the workspace rule, and the layers' state.
Nothing is normalised by the kernels without a GPU."""

import ctypes

import numpy as np
import pytest
import torch
from scipy import sparse

import batchnorm_ref as ref
from deepsphere import _native, gnn_layers
from helpers import rel_err

ENTRY_POINTS = ("dsph_bn_workspace_bytes", "dsph_bn_stats", "dsph_bn_apply", "dsph_bn_backward")
TORCH_ACTS = {"none": lambda t: t, "relu": torch.relu, "elu": torch.nn.functional.elu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}


@pytest.mark.parametrize("act", ref.ACTS)
@pytest.mark.parametrize("affine", [(True, True), (False, False), (True, False), (False, True)], ids=["gamma+shift", "plain", "gamma", "shift"])
def test_yardstick_against_torch_float64_autograd(act, affine):
    """torch.nn.functional.batch_norm on the transposed view + shift + activation, in float64, is the parent's composition."""
    rng = np.random.default_rng(7)
    N, M, F, eps, momentum = 3, 37, 5, 1e-3, 0.1
    y = rng.standard_normal((N, M, F)) * np.array([1.0, 3.0, 1.0, 0.5, 1.0]) + np.array([10.0, 0.0, -10.0, 2.0, 0.0])
    dz = rng.standard_normal((N, M, F))
    gamma = rng.uniform(0.5, 1.5, F) if affine[0] else None
    shift = rng.standard_normal(F) if affine[1] else None
    rm0, rv0 = rng.standard_normal(F), rng.uniform(0.5, 2.0, F)

    ty = torch.tensor(y, dtype=torch.float64, requires_grad=True)
    tg = torch.tensor(np.ones(F) if gamma is None else gamma, dtype=torch.float64, requires_grad=True)
    ts = torch.tensor(np.zeros(F) if shift is None else shift, dtype=torch.float64, requires_grad=True)
    trm, trv = torch.tensor(rm0), torch.tensor(rv0)
    xhat = torch.nn.functional.batch_norm(ty.transpose(1, 2), trm, trv, None, None, True, momentum, eps).transpose(1, 2)
    tz = TORCH_ACTS[act](xhat * tg + ts)
    tz.backward(torch.tensor(dz))

    mean, var, z = ref.bn_forward(y, eps, gamma, shift, act)
    dy, dgamma, dshift = ref.bn_backward(y, dz, eps, gamma, shift, act, z_for_mask=tz.detach().numpy())
    rm, rv = ref.moving_update(rm0, rv0, mean, var, N * M, momentum)
    errs = {"z": rel_err(z, tz.detach().numpy()), "dy": rel_err(dy, ty.grad.numpy()), "dgamma": rel_err(dgamma, tg.grad.numpy()),
            "dshift": rel_err(dshift, ts.grad.numpy()), "running_mean": rel_err(rm, trm.numpy()), "running_var": rel_err(rv, trv.numpy()),
            "mean": rel_err(mean, y.reshape(-1, F).mean(0)), "var": rel_err(var, y.reshape(-1, F).var(0))}
    print(act, affine, {k: f"{v:.1e}" for k, v in errs.items()})
    assert z.shape == y.shape and dy.shape == y.shape and dgamma.shape == (F,) and dshift.shape == (F,)
    for name, e in errs.items():
        assert e <= 1e-12, (name, e)


def test_relu_mask_comes_from_the_output_under_test():
    y = np.array([[1.0], [-1.0], [3.0], [-3.0]])
    dz = np.ones_like(y)
    _, _, z = ref.bn_forward(y, 1e-5, act="relu")
    flipped = z.copy()
    flipped[1, 0] = 1e-9  # an element the code under test rounded to the other side of the kink
    own = ref.bn_backward(y, dz, 1e-5, act="relu")[2]
    other = ref.bn_backward(y, dz, 1e-5, act="relu", z_for_mask=flipped)[2]
    assert own[0] == 2.0 and other[0] == 3.0


def test_entry_points_are_exported_and_bound():
    lib = _native.lib()
    for name in ENTRY_POINTS:
        assert name in _native.SIGNATURES, name
        assert hasattr(lib, name), name
    for name in ("bn_workspace_bytes", "bn_stats", "bn_apply", "bn_backward"):
        assert callable(getattr(_native, name))
    assert lib.dsph_abi_version() == 3


def _partials(rows, F):
    return max(1, min(2048, rows, -(-rows * F // 8192)))


def test_workspace_rule():
    lib = _native.lib()
    shapes = [(1, 1), (2, 4), (15, 3), (576, 5), (1537, 16), (6144, 64), (24576, 70), (36864, 5), (4 * 12 * 1024 * 1024, 64), (10**9, 1000)]
    for rows, F in shapes:
        got = int(lib.dsph_bn_workspace_bytes(rows, F))
        assert got > 0 and got == 16 * F * (_partials(rows, F) + 1) == _native.bn_workspace_bytes(rows, F), (rows, F, got)
    assert _partials(36864, 5) == 23 and _partials(4 * 12 * 1024 * 1024, 64) == 2048
    grid_rows = [1, 2, 3, 15, 576, 1537, 1638, 1639, 8192, 8193, 36864, 10**6, 10**8]
    grid_F = [1, 2, 3, 4, 5, 16, 63, 64, 65, 70, 256, 1025]
    table = np.array([[int(lib.dsph_bn_workspace_bytes(r, F)) for F in grid_F] for r in grid_rows])
    assert (np.diff(table, axis=0) >= 0).all() and (np.diff(table, axis=1) > 0).all(), "monotone in rows and in F"
    for rows, F in [(0, 4), (-1, 4), (4, 0), (4, -2)]:
        assert int(lib.dsph_bn_workspace_bytes(rows, F)) == 0


def test_bad_arguments_are_reported_before_any_device_call():
    """Every case returns DSPH_E_BADARG with a message that names the entry point; none touches HIP, so this runs without a GPU
    (the pointers are host buffers nothing dereferences)."""
    lib = _native.lib()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    null = ctypes.c_void_p()
    ws = 4096

    def stats(y=p, rows=4, F=2, eps=1e-5, mean=p, var=p, rstd=p, rm=null, rv=null, momentum=0.1, w=p, wb=ws):
        return lib.dsph_bn_stats(y, rows, F, eps, mean, var, rstd, null, null, rm, rv, momentum, w, wb, 0, null)

    def apply(y=p, z=p, rows=4, F=2, mean=p, rstd=p, gamma=null, shift=null, act=0):
        return lib.dsph_bn_apply(y, z, rows, F, mean, rstd, gamma, shift, act, 0, null)

    def backward(y=p, z=p, dz=p, mean=p, rstd=p, gamma=null, dy=p, dgamma=null, dshift=null, rows=4, F=2, act=0, w=p, wb=ws):
        return lib.dsph_bn_backward(y, z, dz, mean, rstd, null, null, gamma, dy, dgamma, dshift, rows, F, act, w, wb, 0, null)

    cases = [
        ("bn_stats", lambda: stats(y=null)), ("bn_stats", lambda: stats(mean=null)), ("bn_stats", lambda: stats(var=null)),
        ("bn_stats", lambda: stats(rstd=null)), ("bn_stats", lambda: stats(w=null)),
        ("bn_stats", lambda: stats(rows=0)), ("bn_stats", lambda: stats(rows=-5)), ("bn_stats", lambda: stats(F=0)),
        ("bn_stats", lambda: stats(eps=0.0)), ("bn_stats", lambda: stats(eps=-1e-3)), ("bn_stats", lambda: stats(eps=float("nan"))),
        ("bn_stats", lambda: stats(rm=p, rv=p, momentum=1.5)), ("bn_stats", lambda: stats(rows=1, rm=p, rv=p)),
        ("bn_apply", lambda: apply(y=null)), ("bn_apply", lambda: apply(z=null)), ("bn_apply", lambda: apply(mean=null)),
        ("bn_apply", lambda: apply(rstd=null)), ("bn_apply", lambda: apply(rows=0)), ("bn_apply", lambda: apply(F=0)),
        ("bn_apply", lambda: apply(act=5)), ("bn_apply", lambda: apply(act=-1)),
        ("bn_backward", lambda: backward(y=null)), ("bn_backward", lambda: backward(dz=null)), ("bn_backward", lambda: backward(mean=null)),
        ("bn_backward", lambda: backward(rstd=null)), ("bn_backward", lambda: backward(dy=null)), ("bn_backward", lambda: backward(w=null)),
        ("bn_backward", lambda: backward(rows=0)), ("bn_backward", lambda: backward(F=-1)), ("bn_backward", lambda: backward(act=9)),
        ("bn_backward", lambda: backward(z=null, act=1)),
    ]
    for i, (who, call) in enumerate(cases):
        rc = call()
        msg = _native.last_error()
        assert rc == -1 and who in msg, (i, who, rc, msg)
    # a workspace that is too small is its own code, also before any device call
    assert stats(wb=8) == -4 and "bn_stats" in _native.last_error()
    assert backward(wb=8) == -4 and "bn_backward" in _native.last_error()


def test_wrappers_refuse_host_tensors():
    # (without a GPU: "no GPU is visible", RuntimeError; with one: the map must be a HIP tensor, ValueError -- never a CPU result)
    with pytest.raises((RuntimeError, ValueError), match="no GPU|HIP tensor"):
        _native.bn_stats(torch.zeros(4, 2), 1e-5)
    with pytest.raises((RuntimeError, ValueError), match="no GPU|HIP tensor"):
        _native.bn_apply(torch.zeros(4, 2), torch.zeros(2), torch.ones(2))


def test_layers_keep_their_state_and_the_torch_path_on_the_cpu():
    layer = gnn_layers.Chebyshev(L=sparse.identity(12, format="csr"), K=3, Fout=4, use_bn=True, use_bias=True, activation="relu",
                                 device="cpu")
    layer.build((2, 12, 5))
    assert set(layer.state_dict()) == {"kernel", "bias", "bn.running_mean", "bn.running_var", "bn.num_batches_tracked"}
    assert isinstance(layer.bn, torch.nn.BatchNorm1d) and layer.bn.eps == 1e-5 and layer.bn.momentum == 0.1 and not layer.bn.affine
    # what the kernels do not cover stays with the host framework: CPU tensors, other dtypes, the cumulative average
    y = torch.randn(2, 12, 4)
    assert not gnn_layers._bn_native_ok(layer.bn, y)
    assert not gnn_layers._bn_native_ok(layer.bn, y.double())
    res = gnn_layers.GCNN_ResidualLayer("CHEBY", {"L": sparse.identity(12, format="csr"), "K": 2, "device": "cpu"}, use_bn=True)
    out = res._norm("bn1", y, training=True)  # CPU: torch's batch norm, affine, eps 1e-3, momentum 0.01
    assert isinstance(res.bn1, torch.nn.BatchNorm1d) and res.bn1.eps == 1e-3 and res.bn1.momentum == 0.01 and res.bn1.affine
    assert int(res.bn1.num_batches_tracked) == 1 and out.shape == y.shape
    mean, var, z = ref.bn_forward(y.numpy(), 1e-3)
    assert rel_err(out.detach().numpy(), z) <= 1e-5
    assert set(res.state_dict()) >= {"bn1.weight", "bn1.bias", "bn1.running_mean", "bn1.running_var", "bn1.num_batches_tracked"}
