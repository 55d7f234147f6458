"""CPU tests of the layer-norm path: the float64 yardstick (tests/layernorm_ref.py) against torch's float64 autograd and the
oracle's ``keras_layer_norm``, the three entry points of the C ABI (exported, bound, arguments validated before any HIP call), the
workspace rule, and the layers' state and routing.  Nothing is normalised by the kernels without a GPU."""

import ctypes

import numpy as np
import pytest
import torch
from scipy import sparse

import layernorm_ref as ref
from deepsphere import _native, gnn_layers, gnn_transformers
from helpers import rel_err
from oracle import cheb_oracle as orc

ENTRY_POINTS = ("dsph_ln_workspace_bytes", "dsph_ln_forward", "dsph_ln_backward")


@pytest.mark.parametrize("with_res", [True, False], ids=["res", "plain"])
@pytest.mark.parametrize("affine", [(True, True), (False, False), (True, False), (False, True)], ids=["gamma+beta", "none", "gamma", "beta"])
@pytest.mark.parametrize("rows,d", [(7, 2), (3, 1), (11, 5), (6, 64)])
def test_yardstick_against_torch_float64_autograd(rows, d, affine, with_res):
    """layer_norm(x + res) in float64 with both outputs used downstream is the composition the kernels replace."""
    x, res, dz, dsum, gamma, beta = (v.astype(np.float64) for v in ref.make_data(rows, d))
    eps = 1e-3
    tx = torch.tensor(x, requires_grad=True)
    tr = torch.tensor(res, requires_grad=True)
    tg = torch.tensor(gamma if affine[0] else np.ones(d), requires_grad=True)
    tb = torch.tensor(beta if affine[1] else np.zeros(d), requires_grad=True)
    ta = tx + tr if with_res else tx
    tz = torch.nn.functional.layer_norm(ta, (d,), tg, tb, eps)
    loss = (tz * torch.tensor(dz)).sum() + ((ta * torch.tensor(dsum)).sum() if with_res else 0.0)
    loss.backward()

    z, a = ref.ln_forward(x, eps, gamma if affine[0] else None, beta if affine[1] else None, res if with_res else None)
    da, dgamma, dbeta = ref.ln_backward(a, dz, eps, gamma if affine[0] else None, dsum if with_res else None)
    keras = orc.keras_layer_norm(a, axis=-1, gamma=gamma if affine[0] else None, beta=beta if affine[1] else None, eps=eps)
    errs = {"z": rel_err(z, tz.detach().numpy()), "z vs oracle": rel_err(z, keras), "a": rel_err(a, ta.detach().numpy()),
            "dbeta": rel_err(dbeta, tb.grad.numpy())}
    want_dgamma = tg.grad.numpy()
    if d == 1:  # x^ is identically zero, and so are dgamma and the norm's share of da: absolute comparisons at the scale of their terms
        errs["dgamma"] = float(np.abs(dgamma - want_dgamma).max() / np.abs(dbeta).max())
        errs["da"] = float(np.abs(da - tx.grad.numpy()).max() / (np.abs(dz).max() / np.sqrt(eps)))
    else:
        errs["dgamma"] = rel_err(dgamma, want_dgamma)
        errs["da"] = rel_err(da, tx.grad.numpy())
    if with_res:
        errs["dres - da"] = float(np.abs(tr.grad.numpy() - tx.grad.numpy()).max())
    print((rows, d), affine, with_res, {k: f"{v:.1e}" for k, v in errs.items()})
    assert z.shape == x.shape and da.shape == x.shape and dgamma.shape == (d,) and dbeta.shape == (d,)
    assert np.isfinite(z).all() and np.isfinite(da).all()
    for name, e in errs.items():
        assert e <= 1e-12, (name, e)


def test_entry_points_are_exported_and_bound():
    lib = _native.lib()
    for name in ENTRY_POINTS:
        assert name in _native.SIGNATURES, name
        assert hasattr(lib, name), name
    for name in ("ln_workspace_bytes", "ln_forward", "ln_backward"):
        assert callable(getattr(_native, name))
    assert lib.dsph_abi_version() == 3


def _partials(rows, d):
    return max(1, min(2048, -(-rows // 4), -(-rows * d // 8192)))


def test_workspace_rule():
    lib = _native.lib()
    shapes = [(1, 1), (7, 2), (130, 5), (257, 8), (4099, 64), (300, 256), (9, 1024), (36864, 5), (4 * 786432, 64), (10**9, 1000)]
    for rows, d in shapes:
        got = int(lib.dsph_ln_workspace_bytes(rows, d))
        assert got > 0 and got == 16 * d * _partials(rows, d) == _native.ln_workspace_bytes(rows, d), (rows, d, got)
    assert _partials(36864, 5) == 23 and _partials(4 * 786432, 64) == 2048 and _partials(9, 1024) == 2
    grid_rows = [1, 2, 3, 15, 576, 1537, 1638, 1639, 8192, 8193, 36864, 10**6, 10**8]
    grid_d = [1, 2, 3, 4, 5, 16, 63, 64, 65, 70, 256, 1024]
    table = np.array([[int(lib.dsph_ln_workspace_bytes(r, d)) for d in grid_d] for r in grid_rows])
    assert (np.diff(table, axis=0) >= 0).all() and (np.diff(table, axis=1) > 0).all(), "monotone in rows and in d"
    for rows, d in [(0, 4), (-1, 4), (4, 0), (4, -2), (4, 1025), (4, 1028)]:
        assert int(lib.dsph_ln_workspace_bytes(rows, d)) == 0


def test_bad_arguments_are_reported_before_any_device_call():
    """Every case returns its error code with a message that names the entry point (the overlap cases: and the map that
    overlaps); none touches HIP, so this runs without a GPU (the pointers are made-up addresses nothing dereferences)."""
    lib = _native.lib()
    base, n = 1 << 40, 1 << 30  # made-up addresses a GiB apart: room for every shape below

    def at(i):
        return ctypes.c_void_p(base + i * n)

    X, R, S, Z, W = at(0), at(1), at(2), at(3), at(4)
    null = ctypes.c_void_p()
    ws = 4096

    def fwd(x=X, res=null, s=null, z=Z, rows=4, d=2, eps=1e-3, gamma=null, beta=null):
        return lib.dsph_ln_forward(x, res, s, z, rows, d, eps, gamma, beta, 0, null)

    def bwd(a=X, dz=R, dsum=null, gamma=null, eps=1e-3, da=Z, dgamma=S, dbeta=S, rows=4, d=2, w=W, wb=ws):
        return lib.dsph_ln_backward(a, dz, dsum, gamma, eps, da, dgamma, dbeta, rows, d, w, wb, 0, null)

    inside = ctypes.c_void_p(base + 8)  # 8 bytes into X: overlaps it without being it
    odd = ctypes.c_void_p(base + 4 * n + 4)  # a workspace that is not 8-byte aligned
    cases = [
        ("ln_forward", lambda: fwd(x=null)), ("ln_forward", lambda: fwd(z=null)),
        ("ln_forward", lambda: fwd(res=R)), ("ln_forward", lambda: fwd(s=S)),  # res without sum, sum without res
        ("ln_forward", lambda: fwd(rows=-1)), ("ln_forward", lambda: fwd(d=0)), ("ln_forward", lambda: fwd(d=-3)),
        ("ln_forward", lambda: fwd(d=1025)), ("ln_forward", lambda: fwd(d=1028)),
        ("ln_forward", lambda: fwd(eps=0.0)), ("ln_forward", lambda: fwd(eps=-1e-3)), ("ln_forward", lambda: fwd(eps=float("nan"))),
        ("ln_forward: z overlaps", lambda: fwd(z=X)), ("ln_forward: z overlaps", lambda: fwd(z=inside)),
        ("ln_forward: z overlaps", lambda: fwd(res=R, s=S, z=R)), ("ln_forward: z overlaps", lambda: fwd(res=R, s=S, z=S)),
        ("ln_forward: sum overlaps", lambda: fwd(res=R, s=inside)), ("ln_forward: z overlaps", lambda: fwd(res=R, s=X, z=X)),
        ("ln_backward", lambda: bwd(a=null)), ("ln_backward", lambda: bwd(dz=null)), ("ln_backward", lambda: bwd(da=null)),
        ("ln_backward", lambda: bwd(rows=-2)), ("ln_backward", lambda: bwd(d=0)), ("ln_backward", lambda: bwd(d=1028)),
        ("ln_backward", lambda: bwd(eps=0.0)),
        ("ln_backward: da overlaps", lambda: bwd(da=X)), ("ln_backward: da overlaps", lambda: bwd(da=R)),
        ("ln_backward: da overlaps", lambda: bwd(dsum=Z)), ("ln_backward: da overlaps", lambda: bwd(da=inside)),
        ("ln_backward", lambda: bwd(w=null)), ("ln_backward", lambda: bwd(w=odd)),
    ]
    for i, (who, call) in enumerate(cases):
        rc = call()
        msg = _native.last_error()
        assert rc == -1 and who in msg, (i, who, rc, msg)
    # a workspace that is too small is its own code, also before any device call
    assert bwd(wb=8) == -4 and "ln_backward" in _native.last_error()
    assert bwd(rows=4099, d=64, wb=16 * 64 * _partials(4099, 64) - 1) == -4
    # more than 2^40 rows: not a bad argument, a shape the kernels do not take
    assert fwd(rows=2**40 + 1) == -3 and "ln_forward" in _native.last_error()
    # rows = 0 succeeds without a launch (no GPU here: a launch would fail), in place and with the read-only maps coinciding too
    assert fwd(rows=0) == 0 and fwd(rows=0, res=R, s=X) == 0 and fwd(rows=0, res=R, s=R) == 0
    assert bwd(rows=0) == 0 and bwd(rows=0, dsum=R) == 0 and bwd(rows=0, w=null, wb=0) == 0


def test_wrappers_refuse_host_tensors():
    # (without a GPU: "no GPU is visible", RuntimeError; with one: the map must be a HIP tensor, ValueError -- never a CPU result)
    with pytest.raises((RuntimeError, ValueError), match="no GPU|HIP tensor"):
        _native.ln_forward(torch.zeros(4, 2), None, None, 1e-3)
    with pytest.raises((RuntimeError, ValueError), match="no GPU|HIP tensor"):
        _native.ln_backward(torch.zeros(4, 2), torch.zeros(4, 2), None, 1e-3)


def test_layers_keep_their_state_and_the_torch_path_on_the_cpu():
    L = sparse.identity(12, format="csr")
    res = gnn_layers.GCNN_ResidualLayer("CHEBY", {"L": L, "K": 2, "device": "cpu"}, use_bn=True, norm_type="layer_norm")
    y = torch.randn(2, 12, 4)
    out = res._norm("bn1", y, training=True)  # CPU: torch's layer norm, affine, eps 1e-3
    assert isinstance(res.bn1, torch.nn.LayerNorm) and res.bn1.eps == 1e-3 and res.bn1.normalized_shape == (4,)
    assert set(res.state_dict()) >= {"bn1.weight", "bn1.bias"}
    assert rel_err(out.detach().numpy(), ref.ln_forward(y.numpy(), 1e-3)[0]) <= 1e-5
    # what the kernels do not cover stays with the host framework
    assert not gnn_layers._ln_native_ok(res.bn1, y), "CPU tensors"
    assert not gnn_layers._ln_native_ok(res.bn1, y.double()), "float64"
    wide = torch.nn.LayerNorm(1028, eps=1e-3)
    assert not gnn_layers._ln_native_ok(wide, torch.zeros(2, 3, 1028)), "d = 1028"
    joint = gnn_layers.GCNN_ResidualLayer("CHEBY", {"L": L, "K": 2, "device": "cpu"}, use_bn=True, norm_type="layer_norm",
                                          bn_kwargs={"axis": (1, 2)})
    out = joint._norm("bn1", y, training=True)
    assert joint.bn1.normalized_shape == (12, 4) and not gnn_layers._ln_native_ok(joint.bn1, y), "axis = (1, 2)"
    assert rel_err(out.detach().numpy(), orc.keras_layer_norm(y.numpy().astype(np.float64), axis=(1, 2))) <= 1e-5
    # the same questions asked of tensors that claim a HIP device (meta tensors cannot: the device test comes first) -- the rules
    # on shape alone, through a stand-in
    class OnGpu(torch.Tensor):
        is_cuda = True
    fake = torch.zeros(2, 12, 4).as_subclass(OnGpu)
    assert not gnn_layers._ln_native_ok(joint.bn1, fake), "axis = (1, 2) on a HIP tensor"
    assert not gnn_layers._ln_native_ok(wide, torch.zeros(2, 3, 1028).as_subclass(OnGpu)), "d = 1028 on a HIP tensor"
    nonaxis = gnn_layers.GCNN_ResidualLayer("CHEBY", {"L": L, "K": 2, "device": "cpu"}, use_bn=True, norm_type="layer_norm",
                                            bn_kwargs={"axis": 1})
    with pytest.raises(NotImplementedError):
        nonaxis._norm("bn1", y, training=True)

    block = gnn_transformers.MultiHeadAttention(d_model=16, num_heads=2, dense=True)
    assert isinstance(block.layer_norm1, torch.nn.LayerNorm) and isinstance(block.layer_norm2, torch.nn.LayerNorm)
    assert block.layer_norm1.eps == 1e-3 and block.layer_norm2.eps == 1e-3
    assert set(block.state_dict()) == {"wqkv.weight", "wqkv.bias", "dense.weight", "dense.bias", "layer_norm1.weight", "layer_norm1.bias",
                                       "layer_norm2.weight", "layer_norm2.bias"}
    plain = gnn_transformers.MultiHeadAttention(d_model=16, num_heads=2, use_norm=False, dense=True)
    assert isinstance(plain.layer_norm1, torch.nn.Identity) and isinstance(plain.layer_norm2, torch.nn.Identity)
