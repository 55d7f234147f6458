"""CPU tests of the pseudo-convolution path: the float64 yardstick (tests/pseudoconv_ref.py) against torch's float64 autograd of
Conv1d / ConvTranspose1d and the oracle, the three entry points of the C ABI (exported, bound, arguments validated before any HIP
call), the workspace rule, the Keras arguments of the two layers on CPU tensors, and the reference's autoencoder through
``HealpyGCNN``.  No GEMM runs on the kernels without a GPU."""

import ctypes

import numpy as np
import pytest
import torch

import pseudoconv_ref as ref
from deepsphere import _native, healpy_layers
from deepsphere.healpy_networks import HealpyGCNN
from helpers import rel_err
from oracle import cheb_oracle as orc

ENTRY_POINTS = ("dsph_patch_gemm", "dsph_patch_backward_workspace_bytes", "dsph_patch_epilogue_backward")
TORCH_ACT = {None: lambda t: t, "relu": torch.relu, "elu": torch.nn.functional.elu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}


@pytest.mark.parametrize("act", [None, "relu", "elu", "sigmoid", "tanh"])
@pytest.mark.parametrize("Fin,Fout", [(1, 1), (1, 5), (5, 8), (8, 5), (8, 1)])
@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("transpose", [False, True], ids=["conv", "transpose"])
def test_yardstick_against_torch_float64_autograd(transpose, p, Fin, Fout, act):
    g, N, M = 4 ** p, 2, 48
    rng = np.random.default_rng([p, Fin, Fout, int(transpose)])
    x = rng.standard_normal((N, M, Fin))
    conv = (torch.nn.ConvTranspose1d if transpose else torch.nn.Conv1d)(Fin, Fout, g, stride=g).double()
    with torch.no_grad():
        conv.bias.normal_()
    tx = torch.tensor(x, requires_grad=True)
    ty = TORCH_ACT[act](conv(tx.permute(0, 2, 1))).permute(0, 2, 1)  # channels-first copies in, channels-last out
    weight, bias = conv.weight.detach().numpy(), conv.bias.detach().numpy()
    if transpose:
        X, W = x.reshape(N * M, Fin), ref.conv_transpose_image(weight)
        oracle = orc.healpy_pseudo_conv_transpose(x, np.transpose(weight, (2, 1, 0)), bias, p)
    else:
        X, W = x.reshape(N * M // g, g * Fin), ref.conv_image(weight)
        oracle = orc.healpy_pseudo_conv(x, np.transpose(weight, (2, 1, 0)), bias, p)
    Y = ref.patch_forward(X, W, bias, Fout, act)
    dY = rng.standard_normal(Y.shape)
    ty.backward(torch.tensor(dY.reshape(ty.shape)))
    dX, dW, db = ref.patch_backward(X, W, Y, dY, Fout, act)
    dweight = ref.conv_transpose_image_inverse(dW, Fout, g) if transpose else ref.conv_image_inverse(dW, Fin, g)
    errs = {"y": rel_err(Y.reshape(ty.shape), ty.detach().numpy()),
            "y linear vs oracle": rel_err(ref.patch_forward(X, W, bias, Fout, None).reshape(oracle.shape), oracle),
            "dx": rel_err(dX.reshape(x.shape), tx.grad.numpy()), "dweight": rel_err(dweight, conv.weight.grad.numpy()),
            "dbias": rel_err(db, conv.bias.grad.numpy())}
    print(transpose, p, Fin, Fout, act, {k: f"{v:.1e}" for k, v in errs.items()})
    assert ty.shape == ((N, M * g, Fout) if transpose else (N, M // g, Fout))
    for name, e in errs.items():
        assert e <= 1e-12, (name, e)


def test_entry_points_are_exported_and_bound():
    lib = _native.lib()
    for name in ENTRY_POINTS:
        assert name in _native.SIGNATURES, name
        assert hasattr(lib, name), name
    for name in ("patch_gemm", "patch_backward_workspace_bytes", "patch_epilogue_backward"):
        assert callable(getattr(_native, name))
    assert lib.dsph_abi_version() == 3


def _partials(R, C):
    return max(1, min(2048, -(-R * C // 8192)))


def test_workspace_rule():
    lib = _native.lib()
    grid_R = [1, 2, 3, 130, 257, 4099, 8192, 8193, 10**6, 6291456, 10**9]
    shapes = [(1, 1), (5, 5), (10, 10), (40, 10), (64, 64), (256, 64), (192, 3), (28, 7), (4096, 4096), (4096, 1)]
    table = []
    for R in grid_R:
        row = []
        for C, P in shapes:
            got = int(lib.dsph_patch_backward_workspace_bytes(R, C, P))
            assert got > 0 and got == 8 * P * _partials(R, C) == _native.patch_backward_workspace_bytes(R, C, P), (R, C, P, got)
            row.append(got)
        table.append(row)
    assert (np.diff(np.array(table), axis=0) >= 0).all(), "monotone in R"
    assert _partials(4099, 64) == 33 and _partials(6291456, 64) == 2048 and _partials(3, 5) == 1
    for R, C, P in [(0, 4, 4), (-1, 4, 4), (4, 0, 1), (4, 4, 0), (4, 10, 4), (4, 4097, 1), (2**40 + 1, 4, 4)]:
        assert int(lib.dsph_patch_backward_workspace_bytes(R, C, P)) == 0


def test_bad_arguments_are_reported_before_any_device_call():
    """Every case returns its error code with a message that names the entry point; none touches HIP, so this runs without a
    GPU (the pointers are made-up addresses nothing dereferences)."""
    lib = _native.lib()
    base, n = 1 << 40, 1 << 30  # made-up addresses a GiB apart: room for every shape below

    def at(i):
        return ctypes.c_void_p(base + i * n)

    X, W, B, Y, DY, DZ, DB, WS = (at(i) for i in range(8))
    null = ctypes.c_void_p()

    def gemm(x=X, w=W, b=B, y=Y, R=8, Kd=4, C=6, P=3, act=_native.ACT_ELU, prec=_native.PREC_BF16X6):
        return lib.dsph_patch_gemm(x, w, b, y, R, Kd, C, P, act, prec, 0, null)

    def epi(y=Y, dy=DY, dz=DZ, db=DB, R=8, C=6, P=3, act=_native.ACT_ELU, ws=WS, wb=4096):
        return lib.dsph_patch_epilogue_backward(y, dy, dz, db, R, C, P, act, ws, wb, 0, null)

    inside = lambda ptr: ctypes.c_void_p(ptr.value + 8)  # 8 bytes into a map: overlaps it without being it
    bad = [
        ("patch_gemm", lambda: gemm(x=null)), ("patch_gemm", lambda: gemm(w=null)), ("patch_gemm", lambda: gemm(y=null)),
        ("patch_gemm", lambda: gemm(R=0)), ("patch_gemm", lambda: gemm(R=-4)), ("patch_gemm", lambda: gemm(Kd=0)),
        ("patch_gemm", lambda: gemm(Kd=-1)), ("patch_gemm", lambda: gemm(C=0)), ("patch_gemm", lambda: gemm(P=0)),
        ("patch_gemm", lambda: gemm(P=-3)), ("patch_gemm", lambda: gemm(C=6, P=4)), ("patch_gemm", lambda: gemm(C=3, P=6)),
        ("patch_gemm", lambda: gemm(act=5)), ("patch_gemm", lambda: gemm(act=-1)), ("patch_gemm", lambda: gemm(prec=4)),
        ("patch_gemm", lambda: gemm(prec=-1)),
        ("patch_gemm: y overlaps", lambda: gemm(y=X)), ("patch_gemm: y overlaps", lambda: gemm(y=W)),
        ("patch_gemm: y overlaps", lambda: gemm(y=inside(X))), ("patch_gemm: y overlaps", lambda: gemm(x=inside(Y))),
        ("patch_epilogue_backward", lambda: epi(dy=null)), ("patch_epilogue_backward", lambda: epi(dz=null)),
        ("patch_epilogue_backward", lambda: epi(y=null)),  # an activation needs the stored output
        ("patch_epilogue_backward", lambda: epi(R=0)), ("patch_epilogue_backward", lambda: epi(C=0)), ("patch_epilogue_backward", lambda: epi(P=0)),
        ("patch_epilogue_backward", lambda: epi(C=6, P=4)), ("patch_epilogue_backward", lambda: epi(act=7)),
        ("patch_epilogue_backward: dz overlaps", lambda: epi(dz=Y)), ("patch_epilogue_backward: dz overlaps", lambda: epi(dz=inside(DY))),
        ("patch_epilogue_backward", lambda: epi(ws=null)), ("patch_epilogue_backward", lambda: epi(ws=ctypes.c_void_p(WS.value + 4))),
    ]
    for i, (who, call) in enumerate(bad):
        rc = call()
        msg = _native.last_error()
        assert rc == -1 and who in msg, (i, who, rc, msg)
    # outside the range: not a bad argument, a shape the kernels do not take
    for call in (lambda: gemm(Kd=4097), lambda: gemm(C=4098, P=3), lambda: gemm(R=2**40 + 1)):
        assert call() == -3 and "patch_gemm" in _native.last_error()
    assert epi(C=4098, P=3) == -3 and "patch_epilogue_backward" in _native.last_error()
    # a workspace that is too small is its own code, also before any device call
    assert epi(wb=8) == -4 and "patch_epilogue_backward" in _native.last_error()
    assert epi(R=4099, C=64, P=64, wb=8 * 64 * _partials(4099, 64) - 1) == -4


def test_wrappers_refuse_host_tensors():
    # (without a GPU: "no GPU is visible", RuntimeError; with one: the map must be a HIP tensor, ValueError -- never a CPU result)
    with pytest.raises((RuntimeError, ValueError), match="no GPU|HIP tensor"):
        _native.patch_gemm(torch.zeros(4, 2), torch.zeros(2, 3), None, 3)
    with pytest.raises((RuntimeError, ValueError), match="no GPU|HIP tensor"):
        _native.patch_epilogue_backward(torch.zeros(4, 2), torch.zeros(4, 2), 2, act=_native.ACT_RELU)


# ---- the layers on CPU tensors: the Keras arguments the reference hands to Conv1D / Conv2DTranspose ------------------------------

def _layer_yardstick(layer, x, act):
    """The yardstick on the layer's own weights: -> the (N, M', Fout) map in float64."""
    weight = layer.filter.weight.detach().numpy()
    bias = None if layer.filter.bias is None else layer.filter.bias.detach().numpy()
    N, M, Fin = x.shape
    g = layer.filter_size
    if isinstance(layer, healpy_layers.HealpyPseudoConv_Transpose):
        return ref.patch_forward(x.reshape(N * M, Fin), ref.conv_transpose_image(weight), bias, layer.Fout, act).reshape(N, M * g, layer.Fout)
    return ref.patch_forward(x.reshape(N * M // g, g * Fin), ref.conv_image(weight), bias, layer.Fout, act).reshape(N, M // g, layer.Fout)


def _nonzero_bias(b):
    with torch.no_grad():
        b.copy_(torch.linspace(-0.5, 0.7, b.numel()))


def test_activation_is_applied_on_cpu_tensors():
    x = np.random.default_rng(3).standard_normal((2, 48, 3)).astype(np.float32)
    down = healpy_layers.HealpyPseudoConv(1, 4, activation="relu", bias_initializer=_nonzero_bias)
    y = down(torch.as_tensor(x)).detach().numpy()
    assert y.shape == (2, 12, 4) and (y >= 0).all() and (y == 0).any()
    assert rel_err(y, _layer_yardstick(down, x, "relu")) <= 1e-5
    up = healpy_layers.HealpyPseudoConv_Transpose(1, 4, activation="elu", bias_initializer=_nonzero_bias)
    z = up(torch.as_tensor(x)).detach().numpy()
    assert z.shape == (2, 192, 4) and (z > -1).all() and (z < 0).any()
    assert rel_err(z, _layer_yardstick(up, x, "elu")) <= 1e-5
    # a callable, and a name without a kernel code
    gelu = healpy_layers.HealpyPseudoConv(1, 4, activation="gelu")
    fn = healpy_layers.HealpyPseudoConv(1, 4, activation=torch.nn.functional.gelu)
    gelu(torch.as_tensor(x))
    fn(torch.as_tensor(x))
    fn.filter.load_state_dict(gelu.filter.state_dict())
    assert torch.equal(fn(torch.as_tensor(x)), gelu(torch.as_tensor(x)))
    want = torch.nn.functional.gelu(torch.as_tensor(_layer_yardstick(gelu, x, None))).numpy()
    assert rel_err(gelu(torch.as_tensor(x)).detach().numpy(), want) <= 1e-5


@pytest.mark.parametrize("cls", [healpy_layers.HealpyPseudoConv, healpy_layers.HealpyPseudoConv_Transpose])
def test_use_bias_false_builds_no_bias(cls):
    layer = cls(1, 5, use_bias=False)
    y = layer(torch.zeros(1, 16, 2))
    assert layer.filter.bias is None and set(layer.state_dict()) == {"filter.weight"}
    assert torch.count_nonzero(y) == 0
    with_bias = cls(1, 5, bias_initializer=_nonzero_bias)
    y = with_bias(torch.zeros(1, 16, 2))
    assert set(with_bias.state_dict()) == {"filter.weight", "filter.bias"}
    assert torch.equal(y[0, 0], with_bias.filter.bias.detach()) and torch.equal(y[0, -1], with_bias.filter.bias.detach())


@pytest.mark.parametrize("cls", [healpy_layers.HealpyPseudoConv, healpy_layers.HealpyPseudoConv_Transpose])
def test_keyword_arguments_are_read_or_refused(cls):
    with pytest.raises(ValueError, match="Could not find activation"):
        cls(1, 4, activation="nope")
    with pytest.raises(NotImplementedError, match="padding"):
        cls(1, 4, padding="same")
    with pytest.raises(ValueError, match="precision"):
        cls(1, 4, precision="fp8")
    frozen = cls(1, 4, trainable=False, name="frozen", precision="bf16x3")
    out = frozen(torch.ones(1, 16, 2))
    assert frozen.name == "frozen" and frozen.precision == "bf16x3" and not out.requires_grad
    assert all(not prm.requires_grad for prm in frozen.parameters()) and len(list(frozen.parameters())) == 2
    live = cls(1, 4)
    assert live(torch.ones(1, 16, 2)).requires_grad and all(prm.requires_grad for prm in live.parameters())
    assert live.kwargs == {} and frozen.kwargs["name"] == "frozen"
    # both initialisers are applied in place
    init = cls(1, 4, kernel_initializer=lambda w: torch.nn.init.constant_(w, 0.25), bias_initializer=lambda b: torch.nn.init.constant_(b, -2.0))
    init(torch.ones(1, 16, 2))
    assert (init.filter.weight == 0.25).all() and (init.filter.bias == -2.0).all()


def test_autograd_on_cpu_tensors_follows_the_yardstick():
    x = np.random.default_rng(5).standard_normal((2, 32, 3)).astype(np.float32)
    for cls, act in ((healpy_layers.HealpyPseudoConv, "tanh"), (healpy_layers.HealpyPseudoConv_Transpose, "sigmoid")):
        layer = cls(1, 6, activation=act, bias_initializer=_nonzero_bias)
        tx = torch.tensor(x, requires_grad=True)
        y = layer(tx)
        dy = np.random.default_rng(6).standard_normal(tuple(y.shape)).astype(np.float32)
        y.backward(torch.as_tensor(dy))
        N, M, Fin = x.shape
        g = layer.filter_size
        weight = layer.filter.weight.detach().numpy()
        if cls is healpy_layers.HealpyPseudoConv_Transpose:
            X, W = x.reshape(N * M, Fin), ref.conv_transpose_image(weight)
        else:
            X, W = x.reshape(N * M // g, g * Fin), ref.conv_image(weight)
        Y = ref.patch_forward(X, W, layer.filter.bias.detach().numpy(), 6, act)
        dX, dW, db = ref.patch_backward(X, W, Y, dy.reshape(Y.shape), 6, act)
        dweight = ref.conv_transpose_image_inverse(dW, 6, g) if cls is healpy_layers.HealpyPseudoConv_Transpose else ref.conv_image_inverse(dW, Fin, g)
        assert rel_err(tx.grad.numpy(), dX.reshape(x.shape)) <= 1e-5 and rel_err(layer.filter.weight.grad.numpy(), dweight) <= 1e-5
        assert rel_err(layer.filter.bias.grad.numpy(), db) <= 1e-5


def autoencoder_layers():
    """The autoencoder of the reference's examples/generative_models.ipynb."""
    enc = [healpy_layers.HealpyPseudoConv(p=1, Fout=F, activation="elu") for F in (4, 8, 16)]
    dec = [healpy_layers.HealpyPseudoConv_Transpose(p=1, Fout=F, activation=a) for F, a in ((16, "elu"), (16, "elu"), (1, "linear"))]
    return enc + dec


def autoencoder_yardstick(layers, x):
    """The yardstick chained by hand over the built layers, in float64."""
    h = np.asarray(x, dtype=np.float64)
    for layer, act in zip(layers, ("elu", "elu", "elu", "elu", "elu", None)):
        h = _layer_yardstick(layer, h, act)
    return h


def test_reference_autoencoder_through_the_network_builder():
    torch.manual_seed(0)
    layers = autoencoder_layers()
    model = HealpyGCNN(nside=8, indices=np.arange(768), layers=layers)
    x = np.random.default_rng(7).standard_normal((3, 768, 1)).astype(np.float32)
    y = model(torch.as_tensor(x))
    assert tuple(y.shape) == (3, 768, 1)
    for layer in layers:  # (zero biases would hide a bias that is not applied)
        _nonzero_bias(layer.filter.bias)
    y = model(torch.as_tensor(x)).detach().numpy()
    want = autoencoder_yardstick(layers, x)
    err = rel_err(y, want)
    print(f"autoencoder on CPU tensors vs the yardstick: {err:.2e}")
    assert err <= 1e-5
    # the activations matter: the same weights as a stack of linear maps give another result
    h = np.asarray(x, dtype=np.float64)
    for layer in layers:
        h = _layer_yardstick(layer, h, None)
    assert rel_err(h, want) > 1e-2
