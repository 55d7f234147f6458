"""CPU tests of the dense attention's and Graph_ViT's host side: the argument checks of the C ABI, constructor checks, exports
and the model builder.  No attention is computed without a GPU."""

import ctypes

import numpy as np
import pytest
import torch

import deepsphere
from deepsphere import _native, gnn_transformers, healpy_layers
from deepsphere.healpy_layers import Healpy_ViT, HealpyPool


def _aligned_buffer():
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    return buf, ctypes.c_void_p((p.value + 15) & ~15)


def test_c_abi_forward_names_the_limit_it_refuses():
    """Shapes outside the kernel's return -1 with the limit in the message before anything touches a device."""
    lib = _native.lib()
    buf, p = _aligned_buffer()

    def fwd(ld=8, M=1, heads=2, depth=4, q=p, out=p):
        return lib.dsph_dense_attention_forward(q, p, p, ld, out, None, 1, M, heads, depth, 0, None)

    assert fwd(depth=5) == -1 and "4, 8, 16, 32, 64" in _native.last_error()
    assert fwd(heads=5, depth=64, ld=320) == -1 and "256" in _native.last_error()
    assert fwd(heads=0) == -1
    assert fwd(ld=10) == -1 and "multiple of 4" in _native.last_error()
    assert fwd(ld=4) == -1 and "stride" in _native.last_error()
    assert fwd(q=ctypes.c_void_p(p.value + 4)) == -1 and "16-byte" in _native.last_error()
    assert fwd(q=None) == -1 and "NULL" in _native.last_error()
    assert fwd(out=None) == -1 and "NULL" in _native.last_error()
    assert fwd(M=0) == -1 and "at least 1" in _native.last_error()
    assert fwd(M=-3) == -1 and "at least 1" in _native.last_error()


def test_c_abi_backward_names_the_limit_it_refuses():
    lib = _native.lib()
    buf, p = _aligned_buffer()

    def bwd(ld=8, ld_grad=8, M=1, heads=2, depth=4, q=p, delta=p, dv=p):
        return lib.dsph_dense_attention_backward(q, p, p, ld, p, p, p, delta, p, p, dv, ld_grad, 1, M, heads, depth, 0, None)

    assert bwd(depth=5) == -1 and "4, 8, 16, 32, 64" in _native.last_error()
    assert bwd(heads=5, depth=64, ld=320, ld_grad=320) == -1 and "256" in _native.last_error()
    assert bwd(ld=10) == -1 and "multiple of 4" in _native.last_error()
    assert bwd(ld_grad=10) == -1 and "multiple of 4" in _native.last_error() and "gradients" in _native.last_error()
    assert bwd(ld_grad=4) == -1 and "stride" in _native.last_error()
    assert bwd(q=ctypes.c_void_p(p.value + 4)) == -1 and "16-byte" in _native.last_error()
    assert bwd(dv=ctypes.c_void_p(p.value + 8)) == -1 and "16-byte" in _native.last_error()
    assert bwd(q=None) == -1 and "NULL" in _native.last_error()
    assert bwd(delta=None) == -1 and "NULL" in _native.last_error()
    assert bwd(M=0) == -1 and "at least 1" in _native.last_error()


def test_constructor_checks():
    with pytest.raises(IOError, match="at least 1"):
        gnn_transformers.Graph_ViT(0, 4, 2)
    with pytest.raises((ValueError, AssertionError)):
        gnn_transformers.Graph_ViT(1, 4, 2, n_layers=0)
    with pytest.raises(ValueError):
        gnn_transformers.Graph_ViT(1, 5, 2, activation="no_such_activation")
    layer = gnn_transformers.Graph_ViT(1, key_dim=4, num_heads=2, n_layers=2)  # p = 1: the reference's `not p > 1` refuses it
    assert (layer.p, layer.embed_filter_size, layer.embedding_size, layer.Fout) == (1, 4, 8, 8)
    assert gnn_transformers.Graph_ViT(2, 8, 4).embed_filter_size == 16 and gnn_transformers.Graph_ViT(2, 8, 4).Fout == 32
    assert len(layer.mha_layers) == 2 and all(m.dense_attention and m.nbr is None for m in layer.mha_layers)
    assert layer.embed is None  # built on the first call, like Keras builds it
    layer.build((3, 192, 5))
    names = {n for n, _ in layer.named_parameters()}
    assert {"embed.weight", "embed.bias", "pos_encoder.pos_embedding"} <= names
    for i in range(2):
        for leaf in ("wqkv.weight", "wqkv.bias", "dense.weight", "dense.bias", "layer_norm1.weight", "layer_norm2.bias"):
            assert f"mha_layers.{i}.{leaf}" in names
    # Keras' Conv1D defaults: Glorot-uniform with fans (4^p Fin, 4^p d), zero bias; the position embedding (1, M / 4^p, d)
    assert tuple(layer.embed.weight.shape) == (8, 5, 4) and tuple(layer.embed.bias.shape) == (8,)
    w = layer.embed.weight.detach()
    limit = np.sqrt(6.0 / (4 * 5 + 4 * 8))
    assert float(w.abs().max()) <= limit and float(w.abs().max()) > 0.5 * limit
    assert float(layer.embed.bias.detach().abs().max()) == 0.0
    assert tuple(layer.pos_encoder.pos_embedding.shape) == (1, 48, 8)
    assert float(layer.pos_encoder.pos_embedding.detach().abs().max()) <= np.sqrt(6.0 / 56.0)
    m = layer.mha_layers[0]
    assert float(m.wqkv.bias.detach().abs().max()) == 0.0 and float(m.dense.bias.detach().abs().max()) == 0.0
    assert float(m.wqkv.weight.detach().abs().max()) <= np.sqrt(6.0 / 16.0)
    # without the position embedding and the norms
    bare = gnn_transformers.Graph_ViT(1, 4, 2, positional_encoding=False, layer_norm=False)
    bare.build((1, 48, 3))
    assert not hasattr(bare, "pos_encoder") and isinstance(bare.mha_layers[0].layer_norm1, torch.nn.Identity)
    assert not any("pos_embedding" in n or "layer_norm" in n for n, _ in bare.named_parameters())


def test_pixel_count_and_cpu_inputs_raise():
    layer = gnn_transformers.Graph_ViT(2, 4, 2)
    with pytest.raises(IOError, match="not compatible"):
        layer(torch.zeros(1, 40, 3))  # 40 is no multiple of 16
    with pytest.raises(IOError, match="not compatible"):
        layer.build((1, 40, 3))
    m = gnn_transformers.MultiHeadAttention(8, 2, dense=True)
    t = torch.zeros(1, 48, 8)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(t)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            layer(torch.zeros(1, 48, 3))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            gnn_transformers.scaled_dot_product_attention(t, t, t, 2)
    else:  # (a GPU is visible: CPU tensors are refused all the same, never computed on the host)
        with pytest.raises(ValueError, match="no CPU path"):
            m(t)
        with pytest.raises(ValueError, match="no CPU path"):
            layer(torch.zeros(1, 48, 3))
    # the default block is unchanged: without tables it still points to the ViT path, and now to dense=True
    with pytest.raises(NotImplementedError, match="dense=True"):
        gnn_transformers.MultiHeadAttention(8, 2)(t)


def test_exports():
    assert issubclass(Healpy_ViT, gnn_transformers.Graph_ViT)
    assert "Healpy_ViT" in healpy_layers.__all__ and deepsphere.Healpy_ViT is Healpy_ViT
    assert deepsphere.Graph_ViT is gnn_transformers.Graph_ViT
    assert {"Graph_ViT", "scaled_dot_product_attention"} <= set(gnn_transformers.__all__)
    layer = Healpy_ViT(2, 4, 2, positional_encoding=False, n_layers=3, activation="elu", layer_norm=False)
    assert (layer.p, layer.key_dim, layer.num_heads, layer.positional_encoding, layer.n_layers, layer.activation,
            layer.layer_norm) == (2, 4, 2, False, 3, "elu", False)
    assert layer.Fout == 8 and len(layer.mha_layers) == 3
    for name in ("dsph_dense_attention_forward", "dsph_dense_attention_backward"):
        assert name in _native.SIGNATURES and hasattr(_native.lib(), name)
    assert _native.lib().dsph_abi_version() == 3


def test_healpy_gcnn_counts_the_vit_as_a_reduction():
    model = deepsphere.HealpyGCNN(8, np.arange(768), [Healpy_ViT(2, 4, 2)])
    assert model.nside_out == 2 and len(model.indices_out) == 48 and model.reduction_fac == 4
    assert isinstance(model[0], Healpy_ViT)
    # the pixel set follows the ViT like a pooling layer: a partial map, and a layer behind it at the reduced resolution
    idx = np.arange(64, 192)
    model = deepsphere.HealpyGCNN(8, idx, [Healpy_ViT(1, 4, 2), HealpyPool(1)])
    assert model.nside_out == 2 and np.array_equal(model.indices_out, np.arange(4, 12))
    with pytest.raises(ValueError, match="nside"):
        deepsphere.HealpyGCNN(8, np.arange(768), [Healpy_ViT(4, 4, 2)])  # 8 / 2^4 < 1
