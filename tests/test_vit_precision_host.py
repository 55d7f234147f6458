"""CPU tests of the dense attention's ``precision`` argument: the two ``_prec`` entry points of the C ABI (exports, every
refusal of the plain entry points plus their own two), the constructors' rules, and the numpy emulation of the split arithmetics
(tests/dense_attention_split_ref.py) against the float64 reference.  No attention is computed without a GPU."""

import ctypes

import numpy as np
import pytest

import dense_attention_ref as ref
import dense_attention_split_ref as split_ref
from deepsphere import _native, gnn_transformers
from deepsphere.healpy_layers import Healpy_ViT
from helpers import rel_err

BADARG, UNSUPPORTED = -1, -3
PRECISIONS = [_native.PREC_FP32, _native.PREC_BF16X6, _native.PREC_BF16X3]


def _aligned_buffer():
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    return buf, ctypes.c_void_p((p.value + 15) & ~15)


def test_exports():
    for name in ("dsph_dense_attention_forward_prec", "dsph_dense_attention_backward_prec"):
        assert name in _native.SIGNATURES and hasattr(_native.lib(), name)
    assert _native.lib().dsph_abi_version() == 3


@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_prec_refuses_what_the_plain_entry_point_refuses(precision):
    """The checks of test_vit_host.test_c_abi_forward_names_the_limit_it_refuses under every precision (depth 32, which all three
    run, wherever the depth is not the point)."""
    lib = _native.lib()
    buf, p = _aligned_buffer()

    def fwd(ld=64, M=1, heads=2, depth=32, q=p, out=p):
        return lib.dsph_dense_attention_forward_prec(q, p, p, ld, out, None, 1, M, heads, depth, precision, 0, None)

    assert fwd(depth=5, ld=12) == BADARG and "4, 8, 16, 32, 64" in _native.last_error()
    assert fwd(heads=5, depth=64, ld=320) == BADARG and "256" in _native.last_error()
    assert fwd(heads=0) == BADARG
    assert fwd(ld=66) == BADARG and "multiple of 4" in _native.last_error()
    assert fwd(ld=32) == BADARG and "stride" in _native.last_error()
    assert fwd(q=ctypes.c_void_p(p.value + 4)) == BADARG and "16-byte" in _native.last_error()
    assert fwd(q=None) == BADARG and "NULL" in _native.last_error()
    assert fwd(out=None) == BADARG and "NULL" in _native.last_error()
    assert fwd(M=0) == BADARG and "at least 1" in _native.last_error()
    assert fwd(M=-3) == BADARG and "at least 1" in _native.last_error()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_backward_prec_refuses_what_the_plain_entry_point_refuses(precision):
    lib = _native.lib()
    buf, p = _aligned_buffer()

    def bwd(ld=64, ld_grad=64, M=1, heads=2, depth=32, q=p, delta=p, dv=p):
        return lib.dsph_dense_attention_backward_prec(q, p, p, ld, p, p, p, delta, p, p, dv, ld_grad, 1, M, heads, depth, precision, 0,
                                                      None)

    assert bwd(depth=5, ld=12, ld_grad=12) == BADARG and "4, 8, 16, 32, 64" in _native.last_error()
    assert bwd(heads=5, depth=64, ld=320, ld_grad=320) == BADARG and "256" in _native.last_error()
    assert bwd(ld=66) == BADARG and "multiple of 4" in _native.last_error()
    assert bwd(ld_grad=66) == BADARG and "multiple of 4" in _native.last_error() and "gradients" in _native.last_error()
    assert bwd(ld_grad=32) == BADARG and "stride" in _native.last_error()
    assert bwd(q=ctypes.c_void_p(p.value + 4)) == BADARG and "16-byte" in _native.last_error()
    assert bwd(dv=ctypes.c_void_p(p.value + 8)) == BADARG and "16-byte" in _native.last_error()
    assert bwd(q=None) == BADARG and "NULL" in _native.last_error()
    assert bwd(delta=None) == BADARG and "NULL" in _native.last_error()
    assert bwd(M=0) == BADARG and "at least 1" in _native.last_error()


def test_unknown_precision_and_split_depths_are_refused():
    lib = _native.lib()
    buf, p = _aligned_buffer()

    def fwd(depth, precision):
        return lib.dsph_dense_attention_forward_prec(p, p, p, 2 * depth, p, None, 1, 1, 2, depth, precision, 0, None)

    def bwd(depth, precision):
        return lib.dsph_dense_attention_backward_prec(p, p, p, 2 * depth, p, p, p, p, p, p, p, 2 * depth, 1, 1, 2, depth, precision, 0, None)

    for call in (fwd, bwd):
        for code in (99, -1, _native.PREC_F16X3):
            assert call(32, code) == BADARG and "precision" in _native.last_error()
        for depth in (4, 8, 16):
            for code in (_native.PREC_BF16X6, _native.PREC_BF16X3):
                assert call(depth, code) == UNSUPPORTED and "32, 64" in _native.last_error()


def test_constructors_carry_and_check_the_precision():
    assert gnn_transformers.Graph_ViT(1, 4, 2).mha_layers[0].precision == "fp32"
    assert gnn_transformers.MultiHeadAttention(8, 2).precision == "fp32"
    layer = Healpy_ViT(1, 32, 2, n_layers=3, precision="bf16x3")
    assert layer.precision == "bf16x3" and [m.precision for m in layer.mha_layers] == ["bf16x3"] * 3
    assert gnn_transformers.MultiHeadAttention(128, 2, dense=True, precision="bf16x6").precision == "bf16x6"
    # keyword-last: the positional calls of before mean what they meant
    old = gnn_transformers.Graph_ViT(1, 4, 2, False, 2, "elu", False)
    assert (old.positional_encoding, old.n_layers, old.activation, old.layer_norm, old.precision) == (False, 2, "elu", False, "fp32")
    with pytest.raises(ValueError, match="32 or 64"):
        gnn_transformers.Graph_ViT(1, 4, 2, precision="bf16x3")
    with pytest.raises(ValueError, match="32 or 64"):
        gnn_transformers.MultiHeadAttention(32, 2, dense=True, precision="bf16x6")  # 16 channels per head
    for cls_call in (lambda: gnn_transformers.Graph_ViT(1, 32, 2, precision="fp16"),
                     lambda: Healpy_ViT(1, 32, 2, precision="auto"),
                     lambda: gnn_transformers.MultiHeadAttention(64, 2, dense=True, precision="f16x3")):
        with pytest.raises(ValueError, match="'fp32', 'bf16x6', 'bf16x3'"):
            cls_call()
    with pytest.raises(ValueError, match="dense=True"):
        gnn_transformers.MultiHeadAttention(64, 2, precision="bf16x6")


def test_the_emulation_is_a_usable_yardstick():
    """One small case: the six-term emulation sits at float64 noise of fp32 operands (<= 1e-6 on every quantity), the three-term
    one between it and 1e-4 -- the ordering the GPU test's bound for "bf16x3" (T_fp32 + 3 E_emul) relies on."""
    N, M, heads, depth = 2, 40, 2, 32
    rng = np.random.default_rng(0)
    q, k, v, g = (rng.standard_normal((N, M, heads * depth)).astype(np.float32) for _ in range(4))
    want = ref.attention_grads64(q, k, v, heads, g)
    want_lse = ref.attention_np(q, k, v, heads)[2]
    errs = {}
    for name in ("bf16x6", "bf16x3"):
        out, lse, dq, dk, dv = split_ref.attention(q, k, v, heads, name, g)
        errs[name] = [rel_err(out, want[0]), rel_err(lse, want_lse), rel_err(dq, want[1]), rel_err(dk, want[2]), rel_err(dv, want[3])]
        print(name, " ".join(f"{e:.2e}" for e in errs[name]))
        out_f, lse_f = split_ref.attention(q, k, v, heads, name)
        assert np.array_equal(out_f, out) and np.array_equal(lse_f, lse)
    assert max(errs["bf16x6"]) <= 1e-6
    for e6, e3 in zip(errs["bf16x6"], errs["bf16x3"]):
        assert e6 < e3 <= 1e-4
